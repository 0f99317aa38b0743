#!/usr/bin/env python3
"""Batch FRI next to the most the plain path can do for the same polynomials, alternating in one process (tooling).

The workload: three groups of 64 polynomials, LDE heights 2^20, 2^18 and 2^16 (degrees 2^19 / 2^17 / 2^15 at rate_bits 1), cap
height 4; arity bits [2, 2, 4, 4] (both joins, final polynomial 2^7), 16 proof-of-work bits, 28 queries; every instance opens
its 64 polynomials at zeta and its first 4 at a second point.

  batch     p2hot_batch_oracle_commit (one tree over the three groups), p2hot_batch_fri_commit_dev alone on the three final
            polynomials' sizes, p2hot_batch_prove_openings (one proof)
  separate  one p2hot_commit per group, one p2hot_prove_openings per degree (three trees, three proofs: what a caller could do
            before the batch path existed; the batch verifier does not accept the result)
Wall time of the synchronised calls, host columns in, median of `reps` alternating repetitions after one warm-up; then one
profiled repetition of each side (p2hot_profile_json, HIP events per kernel family; not part of the timings).
usage: bench_batch_fri.py [out.json] [reps]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from plonky2_amd import Engine  # noqa: E402
from plonky2_amd.batch_fri import BatchFriOracle, FriInstanceInfo, batch_fri_committed_trees  # noqa: E402
from plonky2_amd.fri.oracle import FriBatchInfo, PolynomialBatch, prove_openings  # noqa: E402
from plonky2_amd.iop.challenger import Challenger  # noqa: E402
from plonky2_amd.util.synthetic import splitmix_columns_numpy  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
DEGREES, W, RB, CAP = [19, 17, 15], 64, 1, 4
ARITY, POW_BITS, QUERIES = [2, 2, 4, 4], 16, 28
Z0, Z1 = [3, 5], [7, 11]
eng = Engine(0)
groups = [splitmix_columns_numpy(g * W, W, 1 << d) for g, d in enumerate(DEGREES)]
all_cols = [c for g in groups for c in g]
planes = [splitmix_columns_numpy(1000 + 2 * g, 2, 1 << d).T.copy() for g, d in enumerate(DEGREES)]   # [n][2] per instance
res = {k: [] for k in ("batch_commit_ms", "batch_commit_phase_ms", "batch_prove_ms", "separate_commit_ms", "separate_prove_ms")}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def challenger():
    ch = Challenger(eng)
    ch.observe_elements([1, 2, 3])
    return ch


def batch_side(record):
    oracle, t_commit = timed(lambda: BatchFriOracle.from_values(all_cols, RB, False, CAP, engine=eng))
    ch = challenger()
    _, t_phase = timed(lambda: batch_fri_committed_trees(planes, ch, RB, CAP, ARITY, engine=eng))
    inst = [FriInstanceInfo([FriBatchInfo(Z0, [(0, i * W + p) for p in range(W)]), FriBatchInfo(Z1, [(0, i * W + p) for p in range(4)])])
            for i in range(len(DEGREES))]
    ch = challenger()
    _, t_prove = timed(lambda: BatchFriOracle.prove_openings(DEGREES, inst, [oracle], ch, RB, CAP, ARITY, POW_BITS, QUERIES, engine=eng))
    if record:
        res["batch_commit_ms"].append(t_commit)
        res["batch_commit_phase_ms"].append(t_phase)
        res["batch_prove_ms"].append(t_prove)
    del oracle


def plain_arity(d):
    """the same schedule cut to the degree: rounds while the degree bound allows, final polynomial 2^7 where it can be"""
    out, cur = [], d
    for a in ARITY:
        if cur - a >= 7:
            out.append(a)
            cur -= a
    return out


def separate_side(record):
    oracles, t_commit = timed(lambda: [PolynomialBatch.from_values(g, RB, False, CAP, engine=eng) for g in groups])

    def prove_all():
        for o, d in zip(oracles, DEGREES):
            ch = challenger()
            prove_openings([FriBatchInfo(Z0, [(0, p) for p in range(W)]), FriBatchInfo(Z1, [(0, p) for p in range(4)])], [o], ch, RB, CAP,
                           plain_arity(d), POW_BITS, QUERIES, engine=eng)
    _, t_prove = timed(prove_all)
    if record:
        res["separate_commit_ms"].append(t_commit)
        res["separate_prove_ms"].append(t_prove)
    del oracles


for r in range(reps + 1):   # the first repetition warms tables, the block cache and the code objects
    batch_side(r > 0)
    separate_side(r > 0)
profiles = {}
for name, side in (("batch", batch_side), ("separate", separate_side)):
    eng.profile(True)
    eng.profile_results(reset=True)
    side(False)
    profiles[name] = eng.profile_results(reset=True)
    eng.profile(False)
med = {k: float(np.median(v)) for k, v in res.items()}
med["batch_total_ms"] = med["batch_commit_ms"] + med["batch_prove_ms"]
med["separate_total_ms"] = med["separate_commit_ms"] + med["separate_prove_ms"]
med["ratio_separate_over_batch"] = med["separate_total_ms"] / med["batch_total_ms"]
summary = {
    "workload": "3 groups x %d polynomials, degrees 2^%s, rate_bits %d, cap_height %d, arity bits %s, %d PoW bits, %d queries; host columns in"
                % (W, DEGREES, RB, CAP, ARITY, POW_BITS, QUERIES),
    "separate_arity_bits": {str(d): plain_arity(d) for d in DEGREES},
    "device": torch.cuda.get_device_name(0), "reps": reps, "median": med, "samples": res, "profile_ms": profiles,
    "not_measured": "device-resident inputs (the commits here include the host-to-device upload of the columns); other shapes; "
                    "the power-table variant of fold_join_kernel",
}
print(json.dumps(med))
if out_path:
    with open(out_path, "w") as f:
        json.dump(summary, f, indent=1)
