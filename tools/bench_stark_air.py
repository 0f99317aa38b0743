#!/usr/bin/env python3
"""A STARK table's quotient with its own constraints as a constraint program, next to the path a caller had before (tooling).

The workload is tools/bench_stark_lookup.py's: bench.py's starky_k22 shape (2^22 rows, rate 1/2, 2 challenges) widened to 64 trace
columns, one lookup of 16 looking columns and three CTL Zs of 1, 2 and 3 looking entries, constraint_degree 3 (qdf 2, the quotient
coset is the whole LDE), a random trace -- plus a synthetic constraint program of about 200 instructions that reads every column
(per column a product of a local and a next-row value minus a third column or a long-lived shared sum, consumed in turn by constraint /
constraint_transition; two public-input checks under the row filters; one product of degree 3).  The commitments are made once and are not timed.

  a  accs_host     p2hot_stark_quotient_polys with PRECOMPUTED host accumulators: the earlier path without its host evaluation and
                   without the download of the trace LDE -- a lower bound on what a caller paid
  b  host_side     at 2^18 rows only: a, plus the download of the trace LDE, plus the evaluation of the program at every point
                   by NumPy (vectorised Goldilocks arithmetic, one core; a stand-in for the caller's evaluator, named as such)
  c  air           p2hot_stark_quotient_polys_air
  d  kernels       one profiled repetition of c (p2hot_profile_json, HIP events; not part of the timings): stark_air_eval next to
                   stark_aux_terms, and a device-to-device copy of 1 GiB as the run's measured HBM rate
a and c alternate within every repetition; wall time of the synchronised calls, median and spread of `reps` repetitions after one
warm-up of each.  Bytes are algorithmic: the interpreter reads 2 W Nq words (local and next rows) and writes nc Nq.
usage: bench_stark_air.py [out.json] [reps] [log_n]"""
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
from plonky2_amd.starky import air  # noqa: E402
from plonky2_amd.starky.cross_table_lookup import CtlZData, ctl_polys  # noqa: E402
from plonky2_amd.starky.lookup import Column, Filter, GrandProductChallenge, Lookup, lookup_helper_columns  # noqa: E402
from plonky2_amd.starky.prover import compute_quotient_polys, constraint_accs  # noqa: E402
from plonky2_amd.util.synthetic import splitmix_columns_numpy  # noqa: E402

W, RB, CAP, NC, CD = 64, 1, 4, 2, 3
P = 0xFFFFFFFF00000001
COSET_SHIFT, ROOT_2_32 = 14293326489335486720, 7277203076849721926  # field/src/goldilocks_field.rs:80, :87
EPS = np.uint64(0xFFFFFFFF)
M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
PU = np.uint64(P)
eng, reps = None, 5
lookups = [Lookup(list(map(Column.single, range(2, 18))), Column.single(0), Column.single(1))]


def entry(first):
    return [Column.single(first + k) for k in range(3)]


zs = [CtlZData(GrandProductChallenge(3 + k, 1000 + k), [entry(20 + 9 * k + 3 * e) for e in range(k + 1)],
               [Filter.new_simple(Column.single(60 + e)) for e in range(k + 1)]) for k in range(3)]
challenges, alphas, publics = [0x1234567, 0x89ABCDE], [0x1111111, 0x2222222], [0x3333333, 0x4444444]


def synthetic_program():
    b = air.AirBuilder(W, 2)
    lv, nv, pi = b.local_values, b.next_values, b.public_inputs
    b.constraint_first_row(lv[0] - pi[0])
    b.constraint_last_row(lv[1] - pi[1])
    shared = lv[0] + nv[1]  # lives across the whole program, next to the short-lived products
    for c in range(W):
        e = lv[c] * nv[(c + 1) % W] - (shared if c % 4 == 0 else lv[(c + 5) % W])
        (b.constraint if c % 2 else b.constraint_transition)(e)
    b.constraint(lv[2] * lv[3] * nv[4] - ((1 << 63) + 5))
    return b.build()


prog = synthetic_program()
n_arith = sum(1 for i in prog.insns if i[0] < air.CONSTRAINT)


# ------------------------------------------------------------------ the host evaluator of (b): Goldilocks on uint64 vectors
def gl_canon(x):
    return np.where(x >= PU, x - PU, x)


def gl_add(a, b):
    s = a + b
    s = s + EPS * (s < a)
    return gl_canon(s)


def gl_sub(a, b):
    d = a - b
    return d - EPS * (a < b)


def gl_mul(a, b):
    a0, a1, b0, b1 = a & M32, a >> S32, b & M32, b >> S32
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = p01 + (p00 >> S32)
    mid2 = p10 + (mid & M32)
    lo = (mid2 << S32) | (p00 & M32)
    hi = p11 + (mid >> S32) + (mid2 >> S32)
    hh, hl = hi >> S32, hi & M32
    t0 = lo - hh
    t0 = t0 - EPS * (lo < hh)
    t1 = hl * EPS
    r = t0 + t1
    r = r + EPS * (r < t1)
    return gl_canon(r)


def gl_pow_vec(a, e):
    r = np.ones_like(a)
    while e:
        if e & 1:
            r = gl_mul(r, a)
        a = gl_mul(a, a)
        e >>= 1
    return r


def bitrev_perm(bits):
    idx = np.arange(1 << bits, dtype=np.uint64)
    out = np.zeros_like(idx)
    for k in range(bits):
        out |= ((idx >> np.uint64(k)) & np.uint64(1)) << np.uint64(bits - 1 - k)
    return out.astype(np.int64)


def host_frame(log_n, qbits):
    """x, z_last, L_first, L_last at the points of the quotient coset in natural order (set-up, timed apart: the reference keeps
    these as LDEs)"""
    n, m = 1 << log_n, (1 << log_n) << qbits
    w = pow(ROOT_2_32, 1 << (32 - log_n - qbits), P)
    x = np.asarray([COSET_SHIFT], dtype=np.uint64)
    while len(x) < m:
        x = np.concatenate([x, gl_mul(x, np.full(len(x), pow(w, len(x), P), dtype=np.uint64))])
    one = np.ones(m, dtype=np.uint64)
    zh = gl_sub(gl_pow_vec(x, n), one)
    nn = np.full(m, n % P, dtype=np.uint64)
    x_next = np.roll(x, -(1 << qbits))  # w_n x is the point i + 2^qbits
    l_first = gl_mul(zh, gl_pow_vec(gl_mul(nn, gl_sub(x, one)), P - 2))
    l_last = gl_mul(zh, gl_pow_vec(gl_mul(nn, gl_sub(x_next, one)), P - 2))
    z_last = gl_sub(x, np.full(m, pow(pow(ROOT_2_32, 1 << (32 - log_n), P), P - 2, P), dtype=np.uint64))
    return z_last, l_first, l_last


def host_eval(cols_nat, frame, qbits):
    """the program at every point: cols_nat [W][m] in natural order; returns [NC][m]"""
    z_last, l_first, l_last = frame
    m = cols_nat.shape[1]
    nxt = np.roll(cols_nat, -(1 << qbits), axis=1)
    consts = [np.full(m, c, dtype=np.uint64) for c in prog.constants]
    pubs = [np.full(m, p, dtype=np.uint64) for p in publics]
    al = [np.full(m, a, dtype=np.uint64) for a in alphas]
    temps = [None] * prog.num_temps
    acc = [np.zeros(m, dtype=np.uint64) for _ in alphas]

    def opnd(o):
        kind, idx = o >> air.KIND_SHIFT, o & air.INDEX_MASK
        return (cols_nat, nxt, pubs, consts, temps)[kind][idx]
    for op, dst, a, b in prog.insns:
        if op < air.CONSTRAINT:
            temps[dst] = (gl_add, gl_sub, gl_mul)[op](opnd(a), opnd(b))
        else:
            c = opnd(a)
            if op != air.CONSTRAINT:
                c = gl_mul(c, (z_last, l_first, l_last)[op - air.CONSTRAINT_TRANSITION])
            acc = [gl_add(gl_mul(s, x), c) for s, x in zip(acc, al)]
    return np.stack(acc)


def sync():
    torch.cuda.synchronize()


def timed(fn):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return out, (time.perf_counter() - t0) * 1e3


def setup(log_n):
    n = 1 << log_n
    trace = splitmix_columns_numpy(0, W, n)
    bt = PolynomialBatch.from_values(trace, RB, False, CAP, engine=eng, keep_values=True)
    vals = bt.values()
    lcols = lookup_helper_columns(vals, lookups, challenges, CD, engine=eng)
    ccols, _ = ctl_polys(vals, zs, CD, engine=eng)
    ba = PolynomialBatch.from_values(concat_columns(lcols, ccols, eng), RB, False, CAP, engine=eng)
    del vals, lcols, ccols, trace
    return bt, ba


def path_a(bt, ba, accs):
    return compute_quotient_polys(bt, ba, challenges, lookups, zs, alphas, CD, constraint_accs=accs, engine=eng)


def path_c(bt, ba):
    return compute_quotient_polys(bt, ba, challenges, lookups, zs, alphas, CD, air=prog, public_inputs=publics, engine=eng)


def measure(log_n, with_host):
    with np.errstate(over="ignore"):
        return _measure(log_n, with_host)


def _measure(log_n, with_host):
    bt, ba = setup(log_n)
    accs, t_accs = timed(lambda: constraint_accs(bt, prog, publics, alphas, CD, engine=eng))  # also (a)'s precomputed input
    res = {"a_accs_host_ms": [], "c_air_ms": []}
    same = None
    for r in range(reps + 1):  # the first repetition warms tables, the block cache and the code objects
        ca, ta = timed(lambda: path_a(bt, ba, accs))
        cc, tc = timed(lambda: path_c(bt, ba))
        if r == 0:
            same = bool((ca.host() == cc.host()).all())
        else:
            res["a_accs_host_ms"].append(ta)
            res["c_air_ms"].append(tc)
        del ca, cc
    out = {"log_n": log_n, "samples": res, "median_ms": {k: float(np.median(v)) for k, v in res.items()},
           "min_max_ms": {k: [float(min(v)), float(max(v))] for k, v in res.items()}, "chunks_equal": same,
           "constraint_accs_call_ms_first": t_accs,
           "c_over_a": [float(c / a) for a, c in zip(res["a_accs_host_ms"], res["c_air_ms"])]}
    out["c_over_a_median"] = float(np.median(out["c_over_a"]))
    if with_host:
        qbits = 1
        bits = log_n + qbits
        leaves, t_down = timed(lambda: bt.merkle_tree.leaves)          # [N][W], committed order (N = m: rate_bits = qbits)
        t0 = time.perf_counter()
        cols_nat = gl_canon(np.ascontiguousarray(leaves[bitrev_perm(bits)].T))
        t_layout = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        frame = host_frame(log_n, qbits)
        t_frame = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        host_accs = host_eval(cols_nat, frame, qbits)
        t_eval = (time.perf_counter() - t0) * 1e3
        out["host"] = {"lde_download_ms": t_down, "to_natural_columns_ms": t_layout, "selector_setup_ms": t_frame, "numpy_eval_ms": t_eval,
                       "numpy_equals_device": bool((host_accs == accs).all()),
                       "b_host_side_ms": out["median_ms"]["a_accs_host_ms"] + t_down + t_layout + t_eval,
                       "note": "one repetition; NumPy on one core stands in for the caller's evaluator; the selector set-up is not counted"}
        del leaves, cols_nat, host_accs
    return out, bt, ba


def main():
    global eng, reps
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    LOG_N = int(sys.argv[3]) if len(sys.argv) > 3 else 22
    HOST_LOG_N = min(18, LOG_N)
    eng = Engine(0)
    small, bt, ba = measure(HOST_LOG_N, True)
    del bt, ba
    if LOG_N != HOST_LOG_N:
        big, bt, ba = measure(LOG_N, False)
    else:
        big, (bt, ba) = small, setup(LOG_N)
    eng.profile(True)
    eng.profile_results(reset=True)
    path_c(bt, ba)
    sync()
    profile = eng.profile_results(reset=True)
    eng.profile(False)
    del bt, ba

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

    m = (1 << LOG_N) << 1


    def kernel_ms(name):
        v = profile.get(name)
        return v.get("ms") if isinstance(v, dict) else v


    air_ms, aux_ms = kernel_ms("stark_air_eval"), kernel_ms("stark_aux_terms")
    air_bytes = (2 * W + NC) * m * 8
    kern = {"stark_air_eval": {"ms": air_ms, "bytes": air_bytes, "gbs": air_bytes / (air_ms * 1e-3) / 1e9 if air_ms else None,
                               "hbm_frac": air_bytes / (air_ms * 1e-3) / 1e9 / hbm_gbs if air_ms else None,
                               "ns_per_insn_and_point": air_ms * 1e6 / (len(prog.insns) * m) if air_ms else None},
            "stark_aux_terms": {"ms": aux_ms}}
    summary = {
        "workload": "2^%d rows x %d columns, rate_bits %d, %d challenges, constraint_degree %d; 1 lookup of 16 looking columns, CTL Zs of 1 / 2 / 3 entries; "
                    "a constraint program of %d instructions (%d arithmetic, %d consumes), %d temp slots, %d constants"
                    % (LOG_N, W, RB, NC, CD, len(prog.insns), n_arith, len(prog.insns) - n_arith, prog.num_temps, len(prog.constants)),
        "device": torch.cuda.get_device_name(0), "reps": reps, "at_log_n": big, "at_host_log_n": small,
        "hbm_copy_gbs": hbm_gbs, "hbm_copy_samples_ms": copies, "kernels": kern, "profile_ms": profile,
        "not_measured": "a compiled (Rust, rayon, packed) host evaluator; other program lengths and temp counts; block sizes other than 256; "
                        "a satisfied witness (the arithmetic is the same)",
    }
    print(json.dumps({"log_n": LOG_N, "median_ms": big["median_ms"], "c_over_a": big["c_over_a_median"], "chunks_equal": big["chunks_equal"],
                      "host_log_n": HOST_LOG_N, "host": small.get("host"), "host_median_ms": small["median_ms"], "hbm_copy_gbs": hbm_gbs, "kernels": kern}))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
