#!/usr/bin/env python3
"""The middle of M recursion-size proofs through the *_many entry points, next to M rounds of the single-proof calls (tooling).

The shape is bench.py's recursion shape: 2^12 rows, 135 wires of which 80 routed, rate 1/8, cap height 4, 2 challenges, quotient
degree factor 8, the fourteen gates of a recursion circuit under standard_recursion_config (tests/test_recursion_gates.py's set:
4 selectors, 2 gate constants, so constants_sigmas has 86 columns).  The wires are random: at factor 8 the trim keeps every
coefficient, so neither path looks at whether the witness satisfies the gates, and both do the same arithmetic on it.
M witnesses of one circuit; the wires commitments (p2hot_commit_many) and the circuit's own commitment are made once, untimed.

  many     p2hot_partial_products_many -> p2hot_commit_cols_many -> p2hot_quotient_polys_gates_many -> p2hot_commit_cols_many ->
           p2hot_eval_openings_many (the four commitments of every proof at zeta and g * zeta): 5 calls
  single   per proof: p2hot_batch_subgroup_values (the routed wires' values, which the M-form recomputes inside) ->
           p2hot_partial_products -> p2hot_commit_cols -> p2hot_quotient_polys_gates -> p2hot_commit_cols -> p2hot_eval_openings:
           6 M calls on the same inputs.  This is the code the library had before the M-forms.

The two alternate within every repetition, each timed window ends with a device synchronise, every shape is warmed up once.  `equal`
compares the caps of both new commitments and every opening of every proof between the two paths.  The M = 64 line carries the
condition: the M-form's slowest repetition must beat the loop's fastest.
usage: bench_many_middle.py [out.json] [reps]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (PyTorch-ROCm's HIP runtime must be the process's)
from plonky2_amd import Engine  # noqa: E402
from plonky2_amd.fri.oracle import PolynomialBatch, eval_openings, eval_openings_many  # noqa: E402
from plonky2_amd.plonk import prover as pv  # noqa: E402
from tests.test_recursion_gates import _recursion_set  # noqa: E402

LOG_N, W, ROUTED, RB, CAP, NC, QDF = 12, 135, 80, 3, 4, 2, 8
P = 0xFFFFFFFF00000001
COSET_SHIFT, ROOT_2_32 = 14293326489335486720, 7277203076849721926  # field/src/goldilocks_field.rs:80, :87


def _rand(rng, *shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                                  "many_middle.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    eng = Engine(0)
    rng = np.random.default_rng(12)
    n = 1 << LOG_N
    gates, ns = _recursion_set(QDF)
    descriptors = [g.descriptor() for g in gates]
    sigmas_first = ns + 2
    k_is = [pow(COSET_SHIFT, j, P) for j in range(ROUTED)]
    gen = pow(ROOT_2_32, 1 << (32 - LOG_N), P)
    bcs = PolynomialBatch.from_values(_rand(rng, sigmas_first + ROUTED, n), RB, False, CAP, engine=eng)
    ds = bcs.subgroup_values(sigmas_first, ROUTED)
    result = {"shape": {"log_n": LOG_N, "wires": W, "routed": ROUTED, "rate_bits": RB, "cap_height": CAP, "num_challenges": NC,
                        "quotient_degree_factor": QDF, "gates": len(gates)}, "reps": reps, "device": torch.cuda.get_device_name(0), "M": {}}
    for M in (1, 8, 64):
        bw = PolynomialBatch.from_values_many(_rand(rng, M, W, n), RB, CAP, engine=eng)
        betas, gammas, alphas, pihs = _rand(rng, M, NC), _rand(rng, M, NC), _rand(rng, M, NC), _rand(rng, M, 4)
        zetas = _rand(rng, M, 2)
        points = np.asarray([[z, [int(z[0]) * gen % P, int(z[1]) * gen % P]] for z in zetas], dtype=np.uint64)
        gs0 = pv.GateSet(descriptors, ns, 0, (0, 0, 0, 0))
        sets = [pv.GateSet(descriptors, ns, 0, [int(v) for v in pihs[m]]) for m in range(M)]

        def many():
            t0 = time.perf_counter()
            bz = pv.commit_columns_many(pv.all_wires_permutation_partial_products_many(bw, ds, k_is, QDF, betas, gammas, engine=eng), M, RB, CAP, 1, eng)
            chunks = pv.compute_quotient_polys_gates_many(bw, bcs, sigmas_first, bz, k_is, QDF, betas, gammas, alphas, gate_set=gs0,
                                                          public_inputs_hashes=pihs, engine=eng)
            bq = pv.commit_columns_many(chunks, M, RB, CAP, 0, eng)
            opened = eval_openings_many([[bcs, bw[m], bz[m], bq[m]] for m in range(M)], points, eng)
            eng.sync()
            dt = time.perf_counter() - t0
            return dt, [(bz[m].merkle_tree.cap.entries, bq[m].merkle_tree.cap.entries, opened[m]) for m in range(M)]

        def single():
            t0 = time.perf_counter()
            res = []
            for m in range(M):
                zs = pv.all_wires_permutation_partial_products(bw[m].subgroup_values(0, ROUTED), ds, k_is, QDF, betas[m], gammas[m], eng)
                bz = PolynomialBatch.from_values(zs, RB, False, CAP, engine=eng)
                chunks = pv.compute_quotient_polys_gates(bw[m], bcs, sigmas_first, bz, k_is, QDF, betas[m], gammas[m], alphas[m], sets[m], engine=eng)
                bq = PolynomialBatch.from_coeffs(chunks, RB, False, CAP, engine=eng)
                res.append((bz.merkle_tree.cap.entries, bq.merkle_tree.cap.entries, eval_openings([bcs, bw[m], bz, bq], points[m], eng)))
            eng.sync()
            return time.perf_counter() - t0, res

        _, a = many()      # warm-up of both paths at this shape, and the comparison
        _, b = single()
        equal = all((x[0] == y[0]).all() and (x[1] == y[1]).all() and all((u == v).all() for u, v in zip(x[2], y[2])) for x, y in zip(a, b))
        del a, b
        tm, ts = [], []
        for _ in range(reps):
            tm.append(many()[0] * 1e3)
            ts.append(single()[0] * 1e3)
        rec = {"many_ms": float(np.median(tm)), "many_ms_min_max": [min(tm), max(tm)], "single_loop_ms": float(np.median(ts)),
               "single_loop_ms_min_max": [min(ts), max(ts)], "single_over_many": float(np.median(ts) / np.median(tm)), "equal": bool(equal)}
        if M == 64:
            rec["many_slowest_beats_loop_fastest"] = bool(max(tm) < min(ts))
        result["M"][str(M)] = rec
        print("M = %2d: many %.2f ms [%.2f, %.2f], loop of single calls %.2f ms [%.2f, %.2f], ratio %.2f, equal %s"
              % (M, rec["many_ms"], min(tm), max(tm), rec["single_loop_ms"], min(ts), max(ts), rec["single_over_many"], equal), flush=True)
        del bw
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
