#!/usr/bin/env python3
"""The gate constraints of a recursion circuit at the k20 shape (tooling): 135 wires, 80 routed, 2 challenges, quotient degree factor
8, 2^20 rows (2^23 points of the quotient coset); the fourteen gates of a recursive verifier under standard_recursion_config in the
builder's order (by degree), in the selector groups the reference's rule forms (gates/selectors.rs:101-160).

  quotient_all_gates      p2hot_quotient_polys_gates with all fourteen on the device, NULL host residual: wall time, and inside it
                          the scopes "gates_cheap", "gates_recursion" (gates::recursion_gates_kernel), "gates_poseidon_mds"
                          (gates::mds_gate_kernel), "gates_poseidon" and "quotient_perm"
  quotient_old_gates_residual   the same call with only the eight kinds of gates.hpp on the device and the six recursion kinds'
                          sums uploaded as the host residual (2 x 2^23 words): the least the library cost for this circuit before
                          it knew the six, less the CPU evaluation that fills the residual and the leaf copy that evaluation reads
  alone_ms                the kernel scope of each recursion kind described alone (p2hot_gate_sums)
The witness is random: every value is defined for any witness, and with a power-of-two degree factor nothing is trimmed.
usage: bench_recursion_gates.py [out.json] [reps] [log_n]     (out.json defaults to profiles/recursion_gate_quotient.json)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from plonky2_amd import Engine  # noqa: E402
from plonky2_amd.fri.oracle import DeviceColumns, PolynomialBatch  # noqa: E402
from plonky2_amd.plonk import prover as pr  # noqa: E402
from plonky2_amd.util.synthetic import splitmix_columns_numpy  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "recursion_gate_quotient.json")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
log_n = int(sys.argv[3]) if len(sys.argv) > 3 else 20
P = 0xFFFFFFFF00000001
W, NR, NC, QDF, RB, CAP = 135, 80, 2, 8, 3, 4
n = 1 << log_n
eng = Engine(0)
# (name, kind, param0, param1, Gate::degree)
KINDS = [("Noop", pr.GATE_NOOP, 0, 0, 0), ("Constant", pr.GATE_CONSTANT, 2, 0, 1), ("PublicInput", pr.GATE_PUBLIC_INPUT, 0, 0, 1),
         ("PoseidonMds", pr.GATE_POSEIDON_MDS, 0, 0, 1), ("Reducing", pr.GATE_REDUCING, 43, 0, 2), ("ReducingExtension", pr.GATE_REDUCING_EXT, 32, 0, 2),
         ("BaseSum", pr.GATE_BASE_SUM, 63, 2, 2), ("Arithmetic", pr.GATE_ARITHMETIC, 20, 0, 3), ("ArithmeticExtension", pr.GATE_ARITHMETIC_EXT, 10, 0, 3),
         ("MulExtension", pr.GATE_MUL_EXT, 13, 0, 3), ("Exponentiation", pr.GATE_EXPONENTIATION, 66, 0, 4),
         ("RandomAccess", pr.GATE_RANDOM_ACCESS, 4, 4 | 2 << 8, 5), ("CosetInterpolation", pr.GATE_COSET_INTERPOLATION, 4, 6, 6),
         ("Poseidon", pr.GATE_POSEIDON, 0, 0, 7)]
NEW = range(pr.GATE_POSEIDON_MDS, pr.GATE_COSET_INTERPOLATION + 1)
# selector_polynomials: greedily, while group size + the next gate's degree < max_degree = factor + 1
GROUPS, start = [], 0
while start < len(KINDS):
    size = 0
    while start + size < len(KINDS) and size + KINDS[start + size][4] < QDF + 1:
        size += 1
    GROUPS.append((start, start + size))
    start += size
gates = []
for row, (_, kind, p0, p1, _) in enumerate(KINDS):
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
pih = [int(v) for v in rng.integers(0, P, size=4, dtype=np.uint64)]
set_all = pr.GateSet(gates, NS, 0, pih)
set_old = pr.GateSet([g for g in gates if g[0] not in NEW], NS, 0, pih)
set_new = pr.GateSet([g for g in gates if g[0] in NEW], NS, 0, pih)


def wall(fn):
    eng.sync()
    t0 = time.perf_counter()
    r = fn()
    eng.sync()
    return (time.perf_counter() - t0) * 1e3, r


def scopes(fn):
    eng.profile(True)
    eng.profile_results(reset=True)
    fn()
    eng.sync()
    r = eng.profile_results(reset=True)
    eng.profile(False)
    return r


zpp = pr.all_wires_permutation_partial_products(DeviceColumns.upload(wires[:NR], eng), DeviceColumns.upload(cs[SIG_FIRST:], eng), k_is, QDF,
                                                betas, gammas, eng)
b_w = PolynomialBatch.from_values(wires, RB, False, CAP, engine=eng)
b_cs = PolynomialBatch.from_values(cs, RB, False, CAP, engine=eng)
b_zs = PolynomialBatch.from_values(zpp, RB, False, CAP, engine=eng)
del zpp, wires, cs
residual = pr.gate_sums(b_w, b_cs, SIG_FIRST, set_new, QDF, alphas, engine=eng)      # what a CPU evaluation of the six would have produced
on_device = lambda: pr.compute_quotient_polys_gates(b_w, b_cs, SIG_FIRST, b_zs, k_is, QDF, betas, gammas, alphas, set_all, engine=eng)
with_residual = lambda: pr.compute_quotient_polys_gates(b_w, b_cs, SIG_FIRST, b_zs, k_is, QDF, betas, gammas, alphas, set_old, gate_sums=residual,
                                                        engine=eng)
a, b = on_device().host(), with_residual().host()      # warm-up; the two paths agree byte for byte
assert (a == b).all() and a.any()
del a, b
CALLS = (("quotient_all_gates", on_device), ("quotient_old_gates_residual", with_residual))
res = {key: [] for key, _ in CALLS}
for _ in range(reps):                                  # alternating, in one process
    for key, fn in CALLS:
        res[key].append(wall(fn)[0])
stages = {key: scopes(fn) for key, fn in CALLS}
alone = {}
for name, g in zip([k[0] for k in KINDS], gates):
    if g[0] in NEW:
        one = pr.GateSet([g], NS, 0, pih)
        st = scopes(lambda: pr.gate_sums(b_w, b_cs, SIG_FIRST, one, QDF, alphas, engine=eng))
        alone[name] = st["gates_poseidon_mds" if g[0] == pr.GATE_POSEIDON_MDS else "gates_recursion"]["ms"]
med = {k: float(np.median(v)) for k, v in res.items()}
st = stages["quotient_all_gates"]
summary = {
    "workload": "%d wires, %d routed, %d challenges, quotient degree factor %d, 2^%d rows (2^%d points), the 14 gate kinds of a recursion "
                "circuit in %d selector groups %s; random witness" % (W, NR, NC, QDF, log_n, log_n + 3, NS, GROUPS),
    "device": torch.cuda.get_device_name(0), "reps": reps,
    "median_call_ms": med, "samples_call_ms": res, "stages": stages,
    "kernel_ms": {k: st[k]["ms"] for k in ("gates_cheap", "gates_recursion", "gates_poseidon_mds", "gates_poseidon", "quotient_perm")},
    "alone_ms": alone,
    "ratio_all_gates_call_to_old_gates_residual_call": med["quotient_all_gates"] / med["quotient_old_gates_residual"],
}
print(json.dumps({k: summary[k] for k in ("median_call_ms", "kernel_ms", "alone_ms", "ratio_all_gates_call_to_old_gates_residual_call")}))
with open(out_path, "w") as f:
    json.dump(summary, f, indent=1)
