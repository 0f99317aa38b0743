#!/usr/bin/env python3
"""p2hot_prove_openings_many alone on resident oracles: the fused path next to the side-by-side path (tooling).

The shape is bench.py's recursion shape: 2^12 rows, rate 1/8, cap height 4, four oracles of width 84, 135, 20 and 16 (the M
oracles of a position out of one p2hot_commit_many, made once, untimed), 255 polynomials opened at zeta_j and 2 at g * zeta_j,
reduction arity bits 4, 4, 16 bits of proof of work, 28 queries.  Proof j's transcript has observed j + 1 elements.

  fused         P2HOT_MANY_FUSED=1: one set of launches per group of proofs on the caller's stream
  side_by_side  P2HOT_MANY_FUSED=0: M single-proof chains on up to four sibling contexts with their own host threads (the code
                the library had before the fused path, unchanged)

The variable is read per call, so the two alternate within every repetition of one process.  A timed window is the call itself,
which ends with its own synchronisation; every M is warmed up once on both paths, and that pair of runs is compared byte for byte
(`equal`: every proof buffer, witness and query index, and three challenges drawn from every transcript afterwards).  M = 8 and
M = 64 carry the project's condition for an M-form: the fused path's slowest repetition must beat the side-by-side path's fastest.
usage: bench_prove_openings_many.py [out.json] [reps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (PyTorch-ROCm's HIP runtime must be the process's)
from plonky2_amd import Engine, _lib  # noqa: E402
from plonky2_amd.util.synthetic import splitmix_columns_numpy  # noqa: E402

LOG_N, RB, CAP, WIDTHS, ARITY, POW_BITS, Q = 12, 3, 4, (84, 135, 20, 16), (4, 4), 16, 28
P = 0xFFFFFFFF00000001
ROOT_2_32 = 7277203076849721926  # field/src/goldilocks_field.rs:87
NAMES = ("caps", "final_poly", "initial_leaves", "initial_paths", "step_evals", "step_paths")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "prove_openings_many.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    eng = Engine(0)
    n = 1 << LOG_N
    gen = pow(ROOT_2_32, 1 << (32 - LOG_N), P)
    rng = np.random.default_rng(16)
    at_zeta = [(o, i) for o, w in enumerate(WIDTHS) for i in range(w)]
    at_next = [(2, 0), (2, 1)]
    idx = [((C.c_uint32 * len(l))(*[o for o, _ in l]), (C.c_uint32 * len(l))(*[i for _, i in l]), len(l)) for l in (at_zeta, at_next)]
    arity = (C.c_uint * len(ARITY))(*ARITY)
    fp = _lib.FriParams(RB, CAP, POW_BITS, Q, arity, len(ARITY), 0, 0, 0)
    result = {"shape": {"log_n": LOG_N, "rate_bits": RB, "cap_height": CAP, "widths": list(WIDTHS), "polys_at_zeta": len(at_zeta),
                        "polys_at_g_zeta": len(at_next), "arity_bits": list(ARITY), "pow_bits": POW_BITS, "queries": Q},
              "reps": reps, "device": torch.cuda.get_device_name(0), "M": {}}
    for M in (1, 8, 64):
        handles = []
        for o, w in enumerate(WIDTHS):  # the M oracles of a position: one commitment call, different columns per proof
            cols = [splitmix_columns_numpy(1000 * o + 100000 * m, w, n) for m in range(M)]
            ptrs = (C.c_void_p * (M * w))(*[cols[m][e].ctypes.data for m in range(M) for e in range(w)])
            hs = (C.c_void_p * M)()
            eng.check(eng.lib.p2hot_commit_many(eng.ctx, ptrs, M, w, LOG_N, RB, CAP, 0, None, None, None, hs))
            handles.append(hs)
        lay = _lib.FriProofLayout()
        h0 = (C.c_void_p * len(WIDTHS))(*[handles[o][0] for o in range(len(WIDTHS))])
        eng.check(eng.lib.p2hot_fri_proof_sizes(h0, len(WIDTHS), C.byref(fp), C.byref(lay)))
        zetas = rng.integers(0, P, size=(M, 2), dtype=np.uint64)
        infos = []
        for m in range(M):
            inf = (_lib.FriBatchInfo * 2)()
            z = [int(zetas[m][0]), int(zetas[m][1])]
            for b, pt in enumerate((z, [z[0] * gen % P, z[1] * gen % P])):
                inf[b].point[0], inf[b].point[1] = pt
                inf[b].oracle_index, inf[b].poly_index, inf[b].n_polys = idx[b]
            infos.append(inf)
        bp = (C.POINTER(_lib.FriBatchInfo) * M)(*[C.cast(inf, C.POINTER(_lib.FriBatchInfo)) for inf in infos])
        nb = (C.c_size_t * M)(*([2] * M))
        hs_all = (C.c_void_p * (len(WIDTHS) * M))(*[handles[o][m] for m in range(M) for o in range(len(WIDTHS))])

        def call(fused, keep_output):
            chs = []
            for m in range(M):
                h = C.c_void_p()
                eng.check(eng.lib.p2hot_challenger_create(eng.ctx, C.byref(h)))
                obs = np.arange(m + 1, dtype=np.uint64)
                eng.check(eng.lib.p2hot_challenger_step(h, obs.ctypes.data, obs.size, None, 0))
                chs.append(h)
            bufs = [[np.zeros(max(1, getattr(lay, k + "_words")), dtype=np.uint64) for k in NAMES] for _ in range(M)]
            qidx = [np.zeros(Q, dtype=np.uint64) for _ in range(M)]
            proofs = (_lib.FriProof * M)()
            for m in range(M):
                b = bufs[m]
                proofs[m] = _lib.FriProof(b[0].ctypes.data, b[1].ctypes.data, 0, qidx[m].ctypes.data, b[2].ctypes.data, b[3].ctypes.data,
                                          b[4].ctypes.data, b[5].ctypes.data)
            cp = (C.c_void_p * M)(*chs)
            os.environ["P2HOT_MANY_FUSED"] = "1" if fused else "0"
            eng.sync()
            t0 = time.perf_counter()
            eng.check(eng.lib.p2hot_prove_openings_many(eng.ctx, M, bp, nb, hs_all, len(WIDTHS), cp, C.byref(fp), proofs))
            dt = time.perf_counter() - t0
            out = None
            if keep_output:
                draws = np.zeros((M, 3), dtype=np.uint64)
                for m in range(M):
                    eng.check(eng.lib.p2hot_challenger_step(chs[m], None, 0, draws[m].ctypes.data, 3))
                out = (bufs, qidx, [int(proofs[m].pow_witness) for m in range(M)], draws)
            for h in chs:
                eng.lib.p2hot_challenger_destroy(h)
            return dt, out

        _, a = call(True, True)  # warm-up of both paths at this M, and the comparison
        _, b = call(False, True)
        equal = all((x == y).all() for m in range(M) for x, y in zip(a[0][m], b[0][m])) and all((x == y).all() for x, y in zip(a[1], b[1])) \
            and a[2] == b[2] and bool((a[3] == b[3]).all())
        del a, b
        tf, ts = [], []
        for _ in range(reps):
            tf.append(call(True, False)[0] * 1e3)
            ts.append(call(False, False)[0] * 1e3)
        rec = {"fused_ms": float(np.median(tf)), "fused_ms_min_max": [min(tf), max(tf)], "side_by_side_ms": float(np.median(ts)),
               "side_by_side_ms_min_max": [min(ts), max(ts)], "side_by_side_over_fused": float(np.median(ts) / np.median(tf)),
               "fused_ms_per_proof": float(np.median(tf) / M), "equal": bool(equal), "fused_slowest_beats_side_by_side_fastest": bool(max(tf) < min(ts))}
        result["M"][str(M)] = rec
        print("M = %2d: fused %.2f ms [%.2f, %.2f], side by side %.2f ms [%.2f, %.2f], ratio %.2f, equal %s"
              % (M, rec["fused_ms"], min(tf), max(tf), rec["side_by_side_ms"], min(ts), max(ts), rec["side_by_side_over_fused"], equal), flush=True)
        for hs in handles:
            for m in range(M):
                eng.lib.p2hot_batch_free(hs[m])
    os.environ.pop("P2HOT_MANY_FUSED", None)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
