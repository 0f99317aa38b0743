#!/usr/bin/env python3
"""Two gates' constraints in a plonk quotient three ways: hand-written kinds, gate programs, the host residual (tooling).

The workload: 2^20 rows, 135 wires (80 routed), rate 1/8, quotient degree factor 8, 2 challenges; constants_sigmas = [one selector
polynomial, two gate constants, 80 sigmas]; random columns throughout (at factor 8 nothing is trimmed, so the quotient call does not
depend on a satisfied witness and the arithmetic is the same).  The gates: one ArithmeticExtensionGate of 10 operations and one
BaseSumGate<2> of 63 limbs in one selector group.  The commitments are made once and are not timed.

  base  p2hot_quotient_polys_gates with an empty gate set and no host sums: the permutation argument alone (what every path pays)
  a     the two gates as the hand-written kinds P2HOT_GATE_ARITHMETIC_EXT / P2HOT_GATE_BASE_SUM
  b     the same two gates as gate programs (p2hot_quotient_polys_gate_programs, an empty gate set)
  c     an unknown gate's only route before gate programs: the host gate_sums residual, [2][2^23] words = 128 MiB from pageable host
        memory.  The sums are PRECOMPUTED (by the device): c is charged the upload only, not the caller's CPU evaluation of the gates
        at 2^23 points, nor the read-back of the wires LDE that evaluation needs
base, a, b and c alternate within every repetition; wall time of the synchronised calls (PCIe-inclusive), median and spread of `reps`
repetitions after one warm-up of each.  Kernel times are one profiled repetition of a and of b (p2hot_profile_json, HIP events).
usage: bench_gate_programs.py [out.json] [reps] [log_n]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from plonky2_amd import Engine  # noqa: E402
from plonky2_amd.fri.oracle import PolynomialBatch  # noqa: E402
from plonky2_amd.plonk.gate_program import ExtAlgebra, GateBuilder, GateProgram  # noqa: E402
from plonky2_amd.plonk.prover import GATE_ARITHMETIC_EXT, GATE_BASE_SUM, GateSet, compute_quotient_polys_gates, gate_sums  # noqa: E402
from plonky2_amd.util.synthetic import splitmix_columns_numpy  # noqa: E402

W, NUM_ROUTED, RB, CAP, NC, QDF = 135, 80, 3, 4, 2, 8
NUM_OPS, NUM_LIMBS = 10, 63
P = 0xFFFFFFFF00000001
G = 7  # the multiplicative generator the k_is are powers of
betas, gammas, alphas = [0x1234567, 0x89ABCDE], [0x2345678, 0x9ABCDEF], [0x1111111, 0x2222222]
pih = [11, 22, 33, 44]


def arithmetic_extension(b):
    """arithmetic_extension.rs:92-110"""
    const_0, const_1 = b.constants[0], b.constants[1]
    for i in range(NUM_OPS):
        m0, m1, addend, output = (ExtAlgebra.from_wires(b.wires, 8 * i + 2 * t) for t in range(4))
        for v in (output - ((m0 * m1).scalar_mul(const_0) + addend.scalar_mul(const_1))).to_basefield_array():
            b.constraint(v)


def base_sum_2(b):
    """base_sum.rs:153-170, B = 2"""
    limbs = [b.wires[1 + k] for k in range(NUM_LIMBS)]
    computed_sum = b.constant(0)
    for limb in reversed(limbs):
        computed_sum = computed_sum * 2 + limb
    b.constraint(computed_sum - b.wires[0])
    for limb in limbs:
        b.constraint(limb * (limb - 1))


def traced(fn, row):
    b = GateBuilder(W, 2)
    fn(b)
    return GateProgram(b, row, 0, (0, 2))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    log_n = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    eng = Engine(0)
    n = 1 << log_n
    m = n << 3
    num_prods = -(-NUM_ROUTED // QDF) - 1
    bw = PolynomialBatch.from_values(splitmix_columns_numpy(0, W, n), RB, False, CAP, engine=eng)
    bcs = PolynomialBatch.from_values(splitmix_columns_numpy(200, 1 + 2 + NUM_ROUTED, n), RB, False, CAP, engine=eng)
    bzs = PolynomialBatch.from_values(splitmix_columns_numpy(300, NC * (1 + num_prods), n), RB, False, CAP, engine=eng)
    k_is = [pow(G, j, P) for j in range(NUM_ROUTED)]
    kinds = GateSet([(GATE_ARITHMETIC_EXT, 0, 0, 0, 2, NUM_OPS, 0), (GATE_BASE_SUM, 1, 0, 0, 2, NUM_LIMBS, 2)], 1, 0, pih)
    none = GateSet([], 1, 0, pih)
    programs = [traced(arithmetic_extension, 0), traced(base_sum_2, 1)]
    host_sums = gate_sums(bw, bcs, 3, kinds, QDF, alphas, engine=eng)  # (c)'s precomputed residual: pageable host memory
    sums_equal = bool((gate_sums(bw, bcs, 3, none, QDF, alphas, engine=eng, programs=programs) == host_sums).all())

    def call(gate_set, progs=None, sums=None):
        return compute_quotient_polys_gates(bw, bcs, 3, bzs, k_is, QDF, betas, gammas, alphas, gate_set, gate_sums=sums, engine=eng, programs=progs)
    paths = {"base": lambda: call(none), "a_kinds": lambda: call(kinds), "b_programs": lambda: call(none, programs),
             "c_host_residual": lambda: call(none, None, host_sums)}
    res = {k: [] for k in paths}
    chunks = {}
    for r in range(reps + 1):  # the first repetition warms tables, the block cache and the code objects
        for name, fn in paths.items():
            cols, t = timed(fn)
            if r == 0:
                chunks[name] = cols.host()
            else:
                res[name].append(t)
            del cols
    equal = bool((chunks["a_kinds"] == chunks["b_programs"]).all() and (chunks["a_kinds"] == chunks["c_host_residual"]).all())
    del chunks
    kernels = {}
    for name, scope in (("a_kinds", "gates_cheap"), ("b_programs", "gate_programs")):
        eng.profile(True)
        eng.profile_results(reset=True)
        paths[name]()
        torch.cuda.synchronize()
        prof = eng.profile_results(reset=True)
        eng.profile(False)
        v = prof.get(scope)
        kernels[name] = {"scope": scope, "ms": v.get("ms") if isinstance(v, dict) else v, "quotient_perm_ms": (prof.get("quotient_perm") or {}).get("ms")
                         if isinstance(prof.get("quotient_perm"), dict) else prof.get("quotient_perm"), "profile_ms": prof}
    med = {k: float(np.median(v)) for k, v in res.items()}
    n_insns = [len(p.program.insns) for p in programs]
    summary = {
        "workload": "2^%d rows x %d wires (%d routed), rate_bits %d, factor %d, %d challenges; ArithmeticExtensionGate(%d ops) as a program of %d "
                    "instructions / %d temps, BaseSumGate<2>(%d limbs) as one of %d / %d"
                    % (log_n, W, NUM_ROUTED, RB, QDF, NC, NUM_OPS, n_insns[0], programs[0].program.num_temps, NUM_LIMBS, n_insns[1],
                       programs[1].program.num_temps),
        "device": torch.cuda.get_device_name(0), "reps": reps, "samples_ms": res, "median_ms": med,
        "min_max_ms": {k: [float(min(v)), float(max(v))] for k, v in res.items()},
        "over_base_ms": {k: med[k] - med["base"] for k in med if k != "base"},
        "kernel_ms": {k: v["ms"] for k, v in kernels.items()}, "kernels": kernels,
        "b_over_a_kernel": kernels["b_programs"]["ms"] / kernels["a_kinds"]["ms"] if kernels["a_kinds"]["ms"] and kernels["b_programs"]["ms"] else None,
        "host_residual_bytes": int(NC * m * 8), "chunks_equal": equal, "sums_equal": sums_equal,
        "ns_per_insn_and_point": kernels["b_programs"]["ms"] * 1e6 / (sum(n_insns) * m) if kernels["b_programs"]["ms"] else None,
        "not_measured": "the caller's CPU evaluation of the gates and the read-back of the wires LDE that (c) needs; pinned host memory for (c); "
                        "other gates, program lengths and temp counts; block sizes other than 256",
    }
    print(json.dumps({k: summary[k] for k in ("median_ms", "min_max_ms", "over_base_ms", "kernel_ms", "b_over_a_kernel", "chunks_equal", "sums_equal",
                                              "ns_per_insn_and_point")}))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
