"""BatchFriOracle -- mirror of plonky2/src/batch_fri/oracle.rs:29-192 over libp2hot.

from_values / from_coeffs keep the reference's signature (values, rate_bits, blinding, cap_height, timing, fft_root_table);
`timing` and `fft_root_table` are accepted and ignored, `blinding=True` is not on this path.  An oracle is a
`p2hot_batch_oracle` handle; prove_openings is ONE library call (p2hot_batch_prove_openings).  Marshalling only, in the style of
plonky2_amd.fri.oracle.
"""
import ctypes as C

import numpy as np

from .. import _lib
from ..engine import default_engine
from ..fri.oracle import FriBatchInfo, fri_batch_infos, fri_params, fri_proof_buffers, shape_fri_proof
from ..hash.merkle_tree import MerkleCap


class FriInstanceInfo:
    """fri/structure.rs FriInstanceInfo: the batches (opening point + polynomials) of one instance = one degree"""

    def __init__(self, batches):
        self.batches = [b if isinstance(b, FriBatchInfo) else FriBatchInfo(*b) for b in batches]


class _OracleTree:
    """the oracle's BatchMerkleTree (hash/batch_merkle_tree.rs:17-29) behind the handle: cap, digests, leaf_heights, values,
    open_batch"""

    def __init__(self, owner, cap, cap_height, leaf_heights, widths):
        self._o, self.cap, self.cap_height = owner, MerkleCap(cap), cap_height
        self.leaf_heights, self._widths = leaf_heights, widths
        self._digests = None

    @property
    def digests(self):
        if self._digests is None:
            eng = self._o.engine
            nd = eng.num_digests(self.leaf_heights[0], self.cap_height)
            self._digests = np.zeros((nd, 4), dtype=np.uint64)
            if nd:
                eng.check(eng.lib.p2hot_batch_oracle_digests(self._o._h, self._digests.ctypes.data))
        return self._digests

    def values_many(self, leaf_indices):
        eng = self._o.engine
        idx = np.ascontiguousarray(np.asarray(leaf_indices, dtype=np.uint64).reshape(-1))
        out = np.zeros((len(idx), sum(self._widths)), dtype=np.uint64)
        if out.size:
            eng.check(eng.lib.p2hot_batch_oracle_rows(self._o._h, idx.ctypes.data, len(idx), out.ctypes.data))
        return out

    def values(self, leaf_index):  # batch_merkle_tree.rs:155-164
        row, out, w0 = self.values_many([leaf_index])[0], [], 0
        for w in self._widths:
            out.append(row[w0:w0 + w])
            w0 += w
        return out

    def open_batch_many(self, leaf_indices):
        eng = self._o.engine
        idx = np.ascontiguousarray(np.asarray(leaf_indices, dtype=np.uint64).reshape(-1))
        out = np.zeros((len(idx), self.leaf_heights[0] - self.cap_height, 4), dtype=np.uint64)
        if out.size:
            eng.check(eng.lib.p2hot_batch_oracle_paths(self._o._h, idx.ctypes.data, len(idx), out.ctypes.data))
        return out

    def open_batch(self, leaf_index):  # batch_merkle_tree.rs:133-153
        return self.open_batch_many([leaf_index])[0]


class BatchFriOracle:
    def __init__(self, engine, handle, log_n, rate_bits, cap_height, cap):
        self.engine, self._h = engine, handle
        self._log_n = [int(x) for x in log_n]
        self.rate_bits, self.cap_height, self.blinding = rate_bits, cap_height, False
        self.degree_bits = sorted(set(self._log_n), reverse=True)  # oracle.rs:114-116
        widths, heights = [], []
        for g in range(engine.lib.p2hot_batch_oracle_num_groups(handle)):
            w, d = C.c_size_t(), C.c_uint()
            engine.check(engine.lib.p2hot_batch_oracle_group_info(handle, g, C.byref(w), C.byref(d)))
            widths.append(int(w.value))
            heights.append(int(d.value) + rate_bits)
        self.batch_merkle_tree = _OracleTree(self, cap, cap_height, heights, widths)

    def __del__(self):
        try:
            if self._h and getattr(self.engine, "_ctx", None):
                self.engine.lib.p2hot_batch_oracle_free(self._h)
        except Exception:
            pass
        self._h = None

    @property
    def _W(self):
        return len(self._log_n)

    @property
    def polynomials(self):
        """coefficient form in commit order (oracle.rs:31): a list of host arrays, polynomial c has 2^log_n[c] words"""
        flat = np.zeros(sum(1 << l for l in self._log_n), dtype=np.uint64)
        self.engine.check(self.engine.lib.p2hot_batch_oracle_coeffs(self._h, 0, self._W, flat.ctypes.data))
        out, off = [], 0
        for l in self._log_n:
            out.append(flat[off:off + (1 << l)])
            off += 1 << l
        return out

    @classmethod
    def from_values(cls, values, rate_bits, blinding, cap_height, timing=None, fft_root_table=None, engine=None):
        """oracle.rs:44-66.  values: a list of host arrays (values on H_n of every polynomial), lengths non-increasing"""
        return cls._build(values, rate_bits, blinding, cap_height, True, engine)

    @classmethod
    def from_coeffs(cls, polynomials, rate_bits, blinding, cap_height, timing=None, fft_root_table=None, engine=None):
        """oracle.rs:69-125"""
        return cls._build(polynomials, rate_bits, blinding, cap_height, False, engine)

    @classmethod
    def _build(cls, cols, rate_bits, blinding, cap_height, is_values, engine, flags=0):
        if blinding:
            raise ValueError("blinding is not available on the batch FRI path")
        eng = engine or default_engine()
        host = [np.ascontiguousarray(np.asarray(c, dtype=np.uint64).reshape(-1)) for c in cols]
        logs = [int(c.size).bit_length() - 1 for c in host]
        if any(c.size != 1 << l for c, l in zip(host, logs)):
            raise ValueError("polynomial lengths must be powers of two")  # log2_strict, oracle.rs:79
        W = len(host)
        ptrs = (C.c_void_p * max(W, 1))(*[c.ctypes.data for c in host])
        log_n = (C.c_uint * max(W, 1))(*logs)
        cap = np.zeros((1 << cap_height, 4), dtype=np.uint64)
        h = C.c_void_p()
        eng.check(eng.lib.p2hot_batch_oracle_commit(eng.ctx, ptrs, log_n, W, rate_bits, cap_height, 1 if is_values else 0, flags, None,
                                                    None, cap.ctypes.data, C.byref(h)))
        return cls(eng, h, logs, rate_bits, cap_height, cap)

    @staticmethod
    def prove_openings(degree_bits, instances, oracles, challenger, rate_bits, cap_height, reduction_arity_bits, proof_of_work_bits,
                       num_query_rounds, engine=None, timing=None, final_poly_coeff_len=None, max_num_query_steps=None):
        """BatchFriOracle::prove_openings + batch_fri_proof (oracle.rs:128-192, batch_fri/prover.rs:25-86): one
        p2hot_batch_prove_openings call.  Returns the FriProof-shaped dict of fri.oracle.prove_openings; an initial leaf is
        values(x_index) flattened, its siblings open_batch(x_index)."""
        eng = engine or oracles[0].engine
        fp, arity = fri_params(rate_bits, cap_height, reduction_arity_bits, proof_of_work_bits, num_query_rounds, max_num_query_steps,
                               final_poly_coeff_len)
        Q = int(num_query_rounds)
        keep = []  # arrays referenced by the structs
        insts = (_lib.FriInstance * max(len(instances), 1))()
        for i, inst in enumerate(instances):
            infos = fri_batch_infos(inst.batches, keep)
            keep.append(infos)
            insts[i].batches, insts[i].n_batches = infos, len(inst.batches)
        db = (C.c_uint * max(len(degree_bits), 1))(*[int(d) for d in degree_bits])
        handles = (C.c_void_p * max(len(oracles), 1))(*[o._h for o in oracles])
        lay = _lib.FriProofLayout()
        rc = eng.lib.p2hot_batch_fri_proof_sizes(handles, len(oracles), C.byref(fp), C.byref(lay))
        bufs, qidx, proof = fri_proof_buffers(lay if rc == _lib.OK else None, Q)
        # (inconsistent parameters are reported by the call itself, with the argument named)
        eng.check(eng.lib.p2hot_batch_prove_openings(eng.ctx, db, insts, len(instances), handles, len(oracles), challenger._h,
                                                     C.byref(fp), C.byref(proof)))
        bufs["final_poly"] = bufs["final_poly"][:lay.final_poly_words]
        return shape_fri_proof(bufs, int(proof.pow_witness), qidx, [o._W for o in oracles], oracles[0]._log_n[0] + rate_bits, cap_height,
                               arity, Q)
