#!/usr/bin/env python3
"""The lookup argument at the k20 shape (tooling): 80 routed wires, 2 challenges, quotient degree factor 8, 2^20 rows (2^23 points
of the quotient coset), one 256-entry table whose lookups fill a quarter of the rows.

  lookup_polys            p2hot_lookup_polys on device-resident wires (wall time of the call, and its kernels' profile scope)
  quotient_lookup         p2hot_quotient_polys_lookup: wall time, and the scopes of lookup::lookup_terms_kernel ("quotient_lookup")
                          and of plonk::quotient_perm_kernel ("quotient_perm") inside it
  quotient_plain          p2hot_quotient_polys of the same run on the same three commitments (no lookup terms)
The witness is random: every value is defined for any witness, and with a power-of-two degree factor nothing is trimmed.
usage: bench_lookup.py [out.json] [reps] [log_n]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from plonky2_amd import Engine  # noqa: E402
from plonky2_amd.fri.oracle import DeviceColumns, PolynomialBatch  # noqa: E402
from plonky2_amd.plonk.prover import (all_lookup_polys, all_wires_permutation_partial_products, compute_quotient_polys,  # noqa: E402
                                      compute_quotient_polys_lookup, concat_columns)
from plonky2_amd.util.synthetic import splitmix_columns_numpy  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
log_n = int(sys.argv[3]) if len(sys.argv) > 3 else 20
P = 0xFFFFFFFF00000001
NR, NC, QDF, RB, CAP = 80, 2, 8, 3, 4
LU, LUT, NUM_LUTS, SEL_FIRST = NR // 2, NR // 3, 1, 2
n = 1 << log_n
eng = Engine(0)
wires = splitmix_columns_numpy(1, NR + 3, n)
lu_rows, lut_rows = n // 4, -(-256 // LUT)
rows = [(1, 1 + lu_rows, lu_rows + lut_rows)]          # last_lu, last_lut, first_lut
sel = np.zeros((4 + NUM_LUTS, n), dtype=np.uint64)     # gates/selectors.rs:51-99
sel[0, rows[0][1]:rows[0][2] + 1] = 1
sel[1, rows[0][0]:rows[0][1]] = 1
sel[2, rows[0][2] + 1] = 1
sel[3, rows[0][0]] = 1
sel[4, rows[0][1]] = 1
cs = np.concatenate([splitmix_columns_numpy(2, SEL_FIRST, n), sel, splitmix_columns_numpy(3, NR, n)])
SIG_FIRST = SEL_FIRST + 4 + NUM_LUTS
k_is = [pow(7, j, P) for j in range(NR)]
rng = np.random.default_rng(0)
betas, gammas, alphas = ([int(v) for v in rng.integers(0, P, size=NC, dtype=np.uint64)] for _ in range(3))
deltas = [[int(v) for v in rng.integers(0, P, size=4, dtype=np.uint64)] for _ in range(NC)]
evals = [[int(v) for v in rng.integers(0, P, size=NUM_LUTS, dtype=np.uint64)] for _ in range(NC)]

d_wires = DeviceColumns.upload(wires[:NR], eng)


def wall(fn):
    eng.sync()
    t0 = time.perf_counter()
    r = fn()
    eng.sync()
    return (time.perf_counter() - t0) * 1e3, r


polys = lambda: all_lookup_polys(d_wires, rows, deltas, LU, LUT, QDF - 1, engine=eng)
_, lk = wall(polys)                                    # warm-up, and the polynomials for the commitment
zpp = all_wires_permutation_partial_products(d_wires, DeviceColumns.upload(cs[SIG_FIRST:], eng), k_is, QDF, betas, gammas, eng)
b_w = PolynomialBatch.from_values(wires, RB, False, CAP, engine=eng)
b_cs = PolynomialBatch.from_values(cs, RB, False, CAP, engine=eng)
b_zs = PolynomialBatch.from_values(concat_columns(zpp, lk, eng), RB, False, CAP, engine=eng)
del zpp, lk
with_lookup = lambda: compute_quotient_polys_lookup(b_w, b_cs, SIG_FIRST, b_zs, k_is, QDF, betas, gammas, alphas, LU, LUT, SEL_FIRST,
                                                    deltas, evals, engine=eng)
plain = lambda: compute_quotient_polys(b_w, b_cs, SIG_FIRST, b_zs, k_is, QDF, betas, gammas, alphas, engine=eng)
for fn in (with_lookup, plain):
    wall(fn)
res = {"lookup_polys": [], "quotient_lookup": [], "quotient_plain": []}
for _ in range(reps):                                  # alternating, in one process
    for key, fn in (("lookup_polys", polys), ("quotient_lookup", with_lookup), ("quotient_plain", plain)):
        res[key].append(wall(fn)[0])
stages = {}
for key, fn in (("lookup_polys", polys), ("quotient_lookup", with_lookup), ("quotient_plain", plain)):
    eng.profile(True)
    eng.profile_results(reset=True)
    fn()
    eng.sync()
    stages[key] = eng.profile_results(reset=True)
    eng.profile(False)
med = {k: float(np.median(v)) for k, v in res.items()}
k_lookup = stages["quotient_lookup"]["quotient_lookup"]["ms"]
k_perm = stages["quotient_lookup"]["quotient_perm"]["ms"]
summary = {
    "workload": "%d routed wires, %d challenges, quotient degree factor %d, 2^%d rows (2^%d points), one 256-entry table, %d LookupGate "
                "rows, %d LookupTableGate rows; random witness" % (NR, NC, QDF, log_n, log_n + 3, lu_rows, lut_rows),
    "device": torch.cuda.get_device_name(0), "reps": reps,
    "median_call_ms": med, "samples_call_ms": res, "stages": stages,
    "kernel_ms": {"lookup_terms": k_lookup, "quotient_perm": k_perm, "lookup_polys": stages["lookup_polys"]["lookup_polys"]["ms"]},
    "ratio_lookup_terms_kernel_to_permutation_kernel": k_lookup / k_perm if k_perm else None,
    "ratio_quotient_call_with_lookups_to_plain": med["quotient_lookup"] / med["quotient_plain"],
}
print(json.dumps({k: summary[k] for k in ("median_call_ms", "kernel_ms", "ratio_lookup_terms_kernel_to_permutation_kernel",
                                           "ratio_quotient_call_with_lookups_to_plain")}))
if out_path:
    with open(out_path, "w") as f:
        json.dump(summary, f, indent=1)
