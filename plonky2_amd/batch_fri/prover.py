"""The batch commit phase -- mirror of batch_fri_committed_trees (plonky2/src/batch_fri/prover.rs:88-147) on the GPU
(p2hot_batch_fri_commit_dev).  Marshalling only."""
import ctypes as C

import numpy as np

from ..engine import default_engine
from ..hash.merkle_tree import MerkleTree


def batch_fri_committed_trees(coeffs, challenger, rate_bits, cap_height, reduction_arity_bits, engine=None):
    """coeffs: one [n_j][2] array per instance, the nonzero extension coefficients of its final polynomial, degrees strictly
    decreasing (the reference takes instance 0 as padded coefficients and every instance as LDE values on g * H: both are implicit
    here).  The challenger is advanced like the reference.  Returns (trees, final_coeffs, betas) like fri.prover.fri_committed_trees."""
    eng = engine or challenger.engine or default_engine()
    host = [np.ascontiguousarray(np.asarray(c, dtype=np.uint64)) for c in coeffs]
    if any(c.ndim != 2 or c.shape[1] != 2 for c in host):
        raise ValueError("every instance's coeffs must be [n][2]")
    logs = [int(c.shape[0]).bit_length() - 1 for c in host]
    if any(c.shape[0] != 1 << l for c, l in zip(host, logs)):
        raise ValueError("coefficient counts must be powers of two")
    k = len(host)
    planes = [eng.dev(np.ascontiguousarray(c.T)) for c in host]  # [2][n_j]
    ptrs = (C.c_void_p * max(k, 1))(*[eng.mem.ptr(p) for p in planes])
    log_n = (C.c_uint * max(k, 1))(*logs)
    arity = [int(a) for a in reduction_arity_bits]
    ab = (C.c_uint * max(1, len(arity)))(*arity)
    ncap = 1 << cap_height
    m, sizes = (1 << (logs[0] + rate_bits)) if k else 0, []
    for a in arity:
        nl = m >> a
        sizes.append((m, nl, max(0, 2 * (nl - ncap))))
        m >>= a
    n_final = max(m >> rate_bits, 0)
    leaves = eng.mem.empty(max(1, 2 * sum(s[0] for s in sizes)))
    digests = eng.mem.empty(max(1, 4 * sum(s[2] for s in sizes)))
    caps = np.zeros(max(1, 4 * ncap * len(sizes)), dtype=np.uint64)
    betas = np.zeros((max(1, len(sizes)), 2), dtype=np.uint64)
    final = np.zeros((max(1, n_final), 2), dtype=np.uint64)
    eng.check(eng.lib.p2hot_batch_fri_commit_dev(eng.ctx, ptrs, log_n, k, rate_bits, cap_height, ab, len(arity), challenger._h,
                                                 eng.ptr(leaves), eng.ptr(digests), 1, caps.ctypes.data, betas.ctypes.data,
                                                 final.ctypes.data))
    trees, lo, do = [], 0, 0
    for i, (mi, nl, nd) in enumerate(sizes):
        lv = leaves[lo:lo + 2 * mi].reshape(nl, -1)
        trees.append(MerkleTree(leaves=None, digests=digests[do:do + 4 * nd].reshape(nd, 4) if nd else np.zeros((0, 4), np.uint64),
                                cap=caps[4 * ncap * i:4 * ncap * (i + 1)].reshape(ncap, 4), cap_height=cap_height, n_leaves=nl,
                                leaf_getter=(lambda idx, lv=lv: eng.host(lv[np.asarray(idx, dtype=np.int64)])),
                                engine=eng if nd else None))
        lo += 2 * mi
        do += 4 * nd
    return trees, final[:n_final], betas[:len(sizes)]
