#!/usr/bin/env python3
"""starky's lookup / cross-table-lookup stage on the GPU next to the commitments around it, in one process (tooling).

The workload: bench.py's starky_k22 shape (2^22 rows, rate 1/2, 2 challenges, cap height 4) widened to 64 trace columns, with one
lookup of 16 looking columns (default filters) and three CTL Zs of 1, 2 and 3 looking entries (3 columns each, single-column
filters), constraint_degree 3 (chunks of two; quotient degree factor 2, the quotient coset is the whole LDE).  A random trace: every
value the stage computes is defined for any witness, and at qdf = 2^qbits nothing is trimmed, so the quotient call returns chunks.

  trace_commit   PolynomialBatch.from_values, host columns in, values kept on the device
  lookup_polys   p2hot_stark_lookup_polys      ctl_polys   p2hot_stark_ctl_polys       (device columns in and out)
  aux_commit     p2hot_cols_concat + p2hot_commit_cols of the 24 auxiliary columns
  quotient       p2hot_stark_quotient_polys, NULL residual, chunks out
Wall time of the synchronised calls, median and spread of `reps` repetitions after one warm-up; then one profiled repetition
(p2hot_profile_json, HIP events per kernel family; not part of the timings) and a device-to-device copy of 1 GiB as the run's
measured HBM rate.  Bytes are algorithmic: every distinct column a kernel reads or writes once, 8 bytes per row or coset point.
usage: bench_stark_lookup.py [out.json] [reps] [log_n]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from plonky2_amd import Engine  # noqa: E402
from plonky2_amd.fri.oracle import PolynomialBatch  # noqa: E402
from plonky2_amd.plonk.prover import concat_columns  # noqa: E402
from plonky2_amd.starky.cross_table_lookup import CtlZData, ctl_polys  # noqa: E402
from plonky2_amd.starky.lookup import Column, Filter, GrandProductChallenge, Lookup, lookup_helper_columns  # noqa: E402
from plonky2_amd.starky.prover import compute_quotient_polys  # noqa: E402
from plonky2_amd.util.synthetic import splitmix_columns_numpy  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
LOG_N = int(sys.argv[3]) if len(sys.argv) > 3 else 22
W, RB, CAP, NC, CD = 64, 1, 4, 2, 3
n = 1 << LOG_N
eng = Engine(0)
trace = splitmix_columns_numpy(0, W, n)
lookups = [Lookup(list(map(Column.single, range(2, 18))), Column.single(0), Column.single(1))]


def entry(first):
    return [Column.single(first + k) for k in range(3)]


zs = [CtlZData(GrandProductChallenge(3 + k, 1000 + k), [entry(20 + 9 * k + 3 * e) for e in range(k + 1)],
               [Filter.new_simple(Column.single(60 + e)) for e in range(k + 1)]) for k in range(3)]
challenges, alphas = [0x1234567, 0x89ABCDE], [0x1111111, 0x2222222]
STEPS = ("trace_commit_ms", "lookup_polys_ms", "ctl_polys_ms", "aux_commit_ms", "quotient_ms")
res = {k: [] for k in STEPS}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def one(record):
    bt, t0 = timed(lambda: PolynomialBatch.from_values(trace, RB, False, CAP, engine=eng, keep_values=True))
    vals = bt.values()
    lcols, t1 = timed(lambda: lookup_helper_columns(vals, lookups, challenges, CD, engine=eng))
    (ccols, _), t2 = timed(lambda: ctl_polys(vals, zs, CD, engine=eng))
    ba, t3 = timed(lambda: PolynomialBatch.from_values(concat_columns(lcols, ccols, eng), RB, False, CAP, engine=eng))
    chunks, t4 = timed(lambda: compute_quotient_polys(bt, ba, challenges, lookups, zs, alphas, CD, engine=eng))
    widths = (lcols.width, ccols.width, chunks.width)
    if record:
        for k, t in zip(STEPS, (t0, t1, t2, t3, t4)):
            res[k].append(t)
    del chunks, ba, lcols, ccols, vals, bt
    return widths


for r in range(reps + 1):   # the first repetition warms tables, the block cache and the code objects
    widths = one(r > 0)
eng.profile(True)
eng.profile_results(reset=True)
one(False)
profile = eng.profile_results(reset=True)
eng.profile(False)

# the run's HBM rate: a device-to-device copy, read + write
gib = 1 << 30
src, dst = torch.empty(gib, dtype=torch.uint8, device="cuda"), torch.empty(gib, dtype=torch.uint8, device="cuda")
copies = []
for _ in range(6):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    copies.append(e0.elapsed_time(e1))
hbm_gbs = 2 * gib / (float(np.median(copies[1:])) * 1e-3) / 1e9

# algorithmic bytes: distinct columns read + columns written, once each
m = n << 1                                     # the quotient coset (qbits = 1)
lookup_helpers, ctl_helpers = NC * 8, 0 + 1 + 2
# trace columns of the descriptors above: the lookup reads its 16 looking columns (helpers) and its table and frequencies columns
# (increments; all 18 in the quotient); the CTL Zs read 3 + 6 + 9 = 18 entry columns and the 3 filter columns 60..62
LOOKING, CTL_COLS, CTL_FILTERS, CTL_ZS = 16, 18, 3, 3
bytes_of = {
    # looking columns in, NC * 8 helper columns out; CTLs: entry + filter columns in, 3 helpers + the single-entry Z out
    "stark_helper_rows": {"lookup": (LOOKING + lookup_helpers) * n * 8, "ctl": (CTL_COLS + CTL_FILTERS + ctl_helpers + 1) * n * 8},
    # the helpers in, the increments out (a single-entry Z holds its own already); a lookup reads its table and frequencies columns too
    "stark_increments": {"lookup": (lookup_helpers + 2 + NC) * n * 8, "ctl": (ctl_helpers + 2) * n * 8},
    # chunk totals read the increments, the replay reads and writes them
    "stark_scan": {"lookup": 3 * NC * n * 8, "ctl": 3 * CTL_ZS * n * 8},
    # 18 + 21 trace columns at the local row (no descriptor here has a next-row term), the 24 aux columns, the NC + 3 Zs again at
    # the next row, NC outputs
    "stark_aux_terms": (LOOKING + 2 + CTL_COLS + CTL_FILTERS + lookup_helpers + NC + ctl_helpers + CTL_ZS + NC + CTL_ZS + NC) * m * 8,
}
med = {k: float(np.median(v)) for k, v in res.items()}
spread = {k: [float(min(v)), float(max(v))] for k, v in res.items()}
med["aux_polys_over_aux_commit"] = (med["lookup_polys_ms"] + med["ctl_polys_ms"]) / med["aux_commit_ms"]
kern = {}
for name, b in bytes_of.items():
    ms = profile.get(name, {}).get("ms") if isinstance(profile.get(name), dict) else profile.get(name)
    total = b if isinstance(b, int) else sum(b.values())
    kern[name] = {"bytes": b, "profile": profile.get(name), "hbm_frac": (total / (ms * 1e-3) / 1e9 / hbm_gbs) if ms else None}
summary = {
    "workload": "2^%d rows x %d columns, rate_bits %d, cap_height %d, %d challenges, constraint_degree %d; 1 lookup of 16 looking columns, CTL Zs of "
                "1 / 2 / 3 entries; aux columns %d + %d, %d quotient chunks" % (LOG_N, W, RB, CAP, NC, CD, widths[0], widths[1], widths[2]),
    "device": torch.cuda.get_device_name(0), "reps": reps, "median_ms": med, "min_max_ms": spread, "samples": res,
    "hbm_copy_gbs": hbm_gbs, "hbm_copy_samples_ms": copies, "kernels": kern, "profile_ms": profile,
    "not_measured": "the selector form (closed forms from the cached 1 / (n (x - 1)) table against an LDE of the two selectors); the scan "
                    "chunk size (4 rows per lane, lookup.hpp's); other shapes; a satisfied witness (the arithmetic is the same)",
}
print(json.dumps({"median_ms": med, "hbm_copy_gbs": hbm_gbs, "kernels": {k: v["hbm_frac"] for k, v in kern.items()}}))
if out_path:
    with open(out_path, "w") as f:
        json.dump(summary, f, indent=1)
