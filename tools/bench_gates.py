#!/usr/bin/env python3
"""The standard gates' constraints at the k20 shape (tooling): 135 wires, 80 routed, 2 challenges, quotient degree factor 8, 2^20
rows (2^23 points of the quotient coset); Noop, Constant, PublicInput, BaseSum<2>, Arithmetic, ArithmeticExtension, MulExtension
and Poseidon in three selector groups.

  quotient_gates      p2hot_quotient_polys_gates: wall time, and inside it the scopes of gates::cheap_gates_kernel ("gates_cheap"),
                      gates::poseidon_gate_kernel ("gates_poseidon") and plonk::quotient_perm_kernel ("quotient_perm")
  quotient_host_sums  p2hot_quotient_polys of the same run with host gate_sums uploaded (2 x 2^23 words): the path without the
                      device evaluation, less the CPU evaluation that fills those sums
The witness is random: every value is defined for any witness, and with a power-of-two degree factor nothing is trimmed.
usage: bench_gates.py [out.json] [reps] [log_n]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from plonky2_amd import Engine  # noqa: E402
from plonky2_amd.fri.oracle import DeviceColumns, PolynomialBatch  # noqa: E402
from plonky2_amd.plonk import prover as pr  # noqa: E402
from plonky2_amd.util.synthetic import splitmix_columns_numpy  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
log_n = int(sys.argv[3]) if len(sys.argv) > 3 else 20
P = 0xFFFFFFFF00000001
W, NR, NC, QDF, RB, CAP = 135, 80, 2, 8, 3, 4
n = 1 << log_n
eng = Engine(0)
KINDS = [(pr.GATE_NOOP, 0, 0), (pr.GATE_CONSTANT, 2, 0), (pr.GATE_PUBLIC_INPUT, 0, 0), (pr.GATE_BASE_SUM, 63, 2), (pr.GATE_ARITHMETIC, 20, 0),
         (pr.GATE_ARITHMETIC_EXT, 10, 0), (pr.GATE_MUL_EXT, 13, 0), (pr.GATE_POSEIDON, 0, 0)]
GROUPS = [(0, 4), (4, 7), (7, 8)]
gates = []
for row, (kind, p0, p1) in enumerate(KINDS):
    s = next(k for k, (a, b) in enumerate(GROUPS) if a <= row < b)
    gates.append((kind, row, s, GROUPS[s][0], GROUPS[s][1], p0, p1))
NS = len(GROUPS)
SIG_FIRST = NS + 2
sel = np.full((NS, n), 0xFFFFFFFF, dtype=np.uint64)     # gates/selectors.rs: the row's gate index in its group's column
for i in range(len(gates)):
    sel[gates[i][2], i::len(gates)] = i
wires = splitmix_columns_numpy(1, W, n)
cs = np.concatenate([sel, splitmix_columns_numpy(2, 2, n), splitmix_columns_numpy(3, NR, n)])
k_is = [pow(7, j, P) for j in range(NR)]
rng = np.random.default_rng(0)
betas, gammas, alphas = ([int(v) for v in rng.integers(0, P, size=NC, dtype=np.uint64)] for _ in range(3))
gate_set = pr.GateSet(gates, NS, 0, [int(v) for v in rng.integers(0, P, size=4, dtype=np.uint64)])


def wall(fn):
    eng.sync()
    t0 = time.perf_counter()
    r = fn()
    eng.sync()
    return (time.perf_counter() - t0) * 1e3, r


zpp = pr.all_wires_permutation_partial_products(DeviceColumns.upload(wires[:NR], eng), DeviceColumns.upload(cs[SIG_FIRST:], eng), k_is, QDF,
                                                betas, gammas, eng)
b_w = PolynomialBatch.from_values(wires, RB, False, CAP, engine=eng)
b_cs = PolynomialBatch.from_values(cs, RB, False, CAP, engine=eng)
b_zs = PolynomialBatch.from_values(zpp, RB, False, CAP, engine=eng)
del zpp, wires, cs
host_sums = pr.gate_sums(b_w, b_cs, SIG_FIRST, gate_set, QDF, alphas, engine=eng)      # what a CPU evaluation would have produced
on_device = lambda: pr.compute_quotient_polys_gates(b_w, b_cs, SIG_FIRST, b_zs, k_is, QDF, betas, gammas, alphas, gate_set, engine=eng)
uploaded = lambda: pr.compute_quotient_polys(b_w, b_cs, SIG_FIRST, b_zs, k_is, QDF, betas, gammas, alphas, gate_sums=host_sums, engine=eng)
a, b = on_device().host(), uploaded().host()           # warm-up; the two paths agree byte for byte
assert (a == b).all() and a.any()
del a, b
res = {"quotient_gates": [], "quotient_host_sums": []}
for _ in range(reps):                                  # alternating, in one process
    for key, fn in (("quotient_gates", on_device), ("quotient_host_sums", uploaded)):
        res[key].append(wall(fn)[0])
stages = {}
for key, fn in (("quotient_gates", on_device), ("quotient_host_sums", uploaded)):
    eng.profile(True)
    eng.profile_results(reset=True)
    fn()
    eng.sync()
    stages[key] = eng.profile_results(reset=True)
    eng.profile(False)
med = {k: float(np.median(v)) for k, v in res.items()}
st = stages["quotient_gates"]
summary = {
    "workload": "%d wires, %d routed, %d challenges, quotient degree factor %d, 2^%d rows (2^%d points), 8 gate kinds in %d selector "
                "groups; random witness" % (W, NR, NC, QDF, log_n, log_n + 3, NS),
    "device": torch.cuda.get_device_name(0), "reps": reps,
    "median_call_ms": med, "samples_call_ms": res, "stages": stages,
    "kernel_ms": {"gates_cheap": st["gates_cheap"]["ms"], "gates_poseidon": st["gates_poseidon"]["ms"], "quotient_perm": st["quotient_perm"]["ms"]},
    "ratio_device_gates_call_to_uploaded_host_sums_call": med["quotient_gates"] / med["quotient_host_sums"],
}
print(json.dumps({k: summary[k] for k in ("median_call_ms", "kernel_ms", "ratio_device_gates_call_to_uploaded_host_sums_call")}))
if out_path:
    with open(out_path, "w") as f:
        json.dump(summary, f, indent=1)
