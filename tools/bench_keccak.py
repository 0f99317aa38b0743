#!/usr/bin/env python3
"""Poseidon vs KeccakHash<25> commitments at the C3 wires shape (W = 135, 2^20 rows, rate 3, cap 4), alternating in one
process (tooling).

  device: p2hot_commit_dev / p2hot_commit_keccak_dev on device buffers, timed with HIP events on the context's stream
  host:   p2hot_commit (host pointers: PCIe in, coefficients + digests + cap out), wall time; the Poseidon tree absorbs column
          chunks while later columns are still uploading, the Keccak tree is hashed after the last column
usage: bench_keccak.py [out.json] [reps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from plonky2_amd import Engine, _lib  # noqa: E402
from plonky2_amd.util.synthetic import splitmix_columns_numpy  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
W, log_n, rb, cap, HN = 135, 20, 3, 4, 25
n, N = 1 << log_n, 1 << (log_n + rb)
eng = Engine(0)
cols = splitmix_columns_numpy(0, W, n)
d_cols = eng.dev(cols)
nd = eng.num_digests(log_n + rb, cap)
d_coeffs, d_lde = eng.mem.empty(W, n), eng.mem.empty(W, N)
d_dig, d_cap = eng.mem.zeros(nd, 4), eng.mem.zeros(1 << cap, 4)


def device_commit(hs):
    args = (eng.ctx, eng.ptr(d_cols), n, W, log_n, rb, cap, 1, 0, N, eng.ptr(d_coeffs), n, eng.ptr(d_lde), N, None,
            eng.ptr(d_dig), eng.ptr(d_cap))
    eng.check(eng.lib.p2hot_commit_keccak_dev(*args, hs) if hs else eng.lib.p2hot_commit_dev(*args))


def timed_device(hs):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    device_commit(hs)
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


ptrs = (C.c_void_p * W)(*[cols[c].ctypes.data for c in range(W)])
h_coeffs = np.zeros((W, n), dtype=np.uint64)
h_dig = np.zeros((nd, 4), dtype=np.uint64)
h_cap = np.zeros((1 << cap, 4), dtype=np.uint64)


def timed_host(hs):
    t0 = time.perf_counter()
    eng.check(eng.lib.p2hot_commit(eng.ctx, ptrs, W, log_n, rb, cap, 1, _lib.HASH_KECCAK(hs), h_coeffs.ctypes.data, None,
                                   h_dig.ctypes.data, h_cap.ctypes.data, None))
    return (time.perf_counter() - t0) * 1e3


for hs in (0, HN, 0, HN):  # warm-up: tables, block cache, code objects
    timed_device(hs)
    timed_host(hs)
res = {"poseidon": {"device_ms": [], "host_ms": []}, "keccak25": {"device_ms": [], "host_ms": []}}
for _ in range(reps):
    for hs, key in ((0, "poseidon"), (HN, "keccak25")):
        res[key]["device_ms"].append(timed_device(hs))
        res[key]["host_ms"].append(timed_host(hs))
# the stages of one device commit of each (profile scopes: the LDE, the leaf sponge, the levels)
stages = {}
for hs, key in ((0, "poseidon"), (HN, "keccak25")):
    eng.profile(True)
    eng.profile_results(reset=True)
    device_commit(hs)
    eng.sync()
    stages[key] = eng.profile_results(reset=True)
    eng.profile(False)
summary = {
    "workload": "C3 wires shape: from_values W=%d, 2^%d rows, rate_bits %d, cap_height %d; PoseidonHash vs KeccakHash<%d>"
                % (W, log_n, rb, cap, HN),
    "device": torch.cuda.get_device_name(0), "reps": reps,
    "median_ms": {k: {m: float(np.median(v[m])) for m in v} for k, v in res.items()},
    "samples_ms": res, "stages": stages,
}
print(json.dumps(summary["median_ms"]))
if out_path:
    with open(out_path, "w") as f:
        json.dump(summary, f, indent=1)
