#!/usr/bin/env python3
"""The opening proof of the Keccak config next to the Poseidon one at the C3 shape's FRI (the wires oracle: W = 135, 2^20 rows,
rate 3, cap 4; arity 16 x4, 16 proof-of-work bits, 28 queries), alternating in one process (tooling).

  prove_ms      p2hot_prove_openings, wall time of the synchronised call
  duplex_us     one duplex of the Keccak / Poseidon challenger: HIP-event time of ONE challenger kernel that observes 8 * 64
                elements (64 dependent duplexes), divided by 64
  grind         p2hot_fri_pow at 22 bits: the candidates the kernels evaluated (every chunk up to the one that holds the witness)
                per second of wall time
usage: bench_keccak_fri.py [out.json] [reps]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from plonky2_amd import Engine  # noqa: E402
from plonky2_amd.fri.oracle import FriBatchInfo, PolynomialBatch, prove_openings  # noqa: E402
from plonky2_amd.fri.prover import fri_proof_of_work  # noqa: E402
from plonky2_amd.hash.keccak import KeccakHash  # noqa: E402
from plonky2_amd.iop.challenger import Challenger  # noqa: E402
from plonky2_amd.util.synthetic import splitmix_columns_numpy  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
W, log_n, rb, cap, HN = 135, 20, 3, 4, 25
ARITY, POW_BITS, QUERIES, GRIND_BITS = [4, 4, 4, 4], 16, 28, 22
eng = Engine(0)
cols = splitmix_columns_numpy(0, W, 1 << log_n)
hashers = {"poseidon": None, "keccak25": KeccakHash(HN, engine=eng)}
batches = [FriBatchInfo([3, 5], [(0, p) for p in range(W)]), FriBatchInfo([7, 11], [(0, p) for p in range(4)])]
res = {k: {"prove_ms": [], "duplex_us": [], "grind_cand_per_s": []} for k in hashers}


def candidates_evaluated(witness, bits):
    """pow_search_dev's chunks: 2^min(18, max(14, bits)) candidates, doubling up to 2^24; later chunks retire at once"""
    chunk, end = 1 << min(18, max(14, bits)), 0
    while end <= witness:
        end += chunk
        chunk = min(2 * chunk, 1 << 24)
    return end


for key, hasher in hashers.items():
    oracle = PolynomialBatch.from_values(cols, rb, False, cap, engine=eng, hasher=hasher)
    for r in range(reps + 1):  # the first repetition warms tables, the block cache and the code objects
        ch = Challenger(eng, hasher=hasher)
        ch.observe_elements([1, 2, 3])
        t = {}
        prove_openings(batches, [oracle], ch, rb, cap, ARITY, POW_BITS, QUERIES, engine=eng, timing=t)
        s = torch.cuda.current_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        obs = np.arange(1, 8 * 64 + 1, dtype=np.uint64)
        e0.record(s)
        eng.check(eng.lib.p2hot_challenger_step(ch._h, obs.ctypes.data, obs.size, None, 0))
        e1.record(s)
        e1.synchronize()
        t0 = time.perf_counter()
        w = fri_proof_of_work(ch, GRIND_BITS, engine=eng)
        dt = time.perf_counter() - t0
        if r:
            res[key]["prove_ms"].append(t["prove_openings"])
            res[key]["duplex_us"].append(e0.elapsed_time(e1) * 1e3 / 64)
            res[key]["grind_cand_per_s"].append(candidates_evaluated(w, GRIND_BITS) / dt)
    del oracle
    eng.check(eng.lib.p2hot_ctx_trim(eng.ctx))
summary = {
    "workload": "prove_openings of one oracle W=%d, 2^%d rows, rate_bits %d, cap_height %d, arity 16 x%d, %d PoW bits, %d queries; "
                "PoseidonHash vs KeccakHash<%d> (transcript, round trees, grind)" % (W, log_n, rb, cap, len(ARITY), POW_BITS, QUERIES, HN),
    "device": torch.cuda.get_device_name(0), "reps": reps,
    "median": {k: {m: float(np.median(v[m])) for m in v} for k, v in res.items()},
    "samples": res,
}
print(json.dumps(summary["median"]))
if out_path:
    with open(out_path, "w") as f:
        json.dump(summary, f, indent=1)
