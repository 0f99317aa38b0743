"""BatchMerkleTree -- mirror of plonky2/src/hash/batch_merkle_tree.rs (struct :17-29, new :35-130, open_batch :133-153,
values :155-164) with the tree built by libp2hot on the GPU (p2hot_batch_merkle_dev).  Marshalling only.
"""
import ctypes as C

import numpy as np

from ..engine import default_engine
from .merkle_tree import MerkleCap


def _tables(eng, groups):
    """the (d_groups, strides, widths, log_heights) argument tables of the p2hot_batch_merkle_*_dev calls"""
    k = len(groups)
    ptrs = (C.c_void_p * max(k, 1))(*[eng.mem.ptr(g) if g.shape[0] else None for g in groups])
    strides = (C.c_size_t * max(k, 1))(*[g.shape[1] for g in groups])
    widths = (C.c_size_t * max(k, 1))(*[g.shape[0] for g in groups])
    logs = (C.c_uint * max(k, 1))(*[int(g.shape[1]).bit_length() - 1 for g in groups])
    return ptrs, strides, widths, logs


class BatchMerkleTree:
    """leaves: the matrices, tallest first; digests [2 (2^h_0 - 2^cap_height)][4]: the segments' digest arrays back to back;
    cap [2^cap_height][4]; leaf_heights: log2 of every matrix's height.

    The matrices live on the device column-major ([W_j][2^h_j]); `leaves` copies them back row-major on demand.
    """

    def __init__(self, engine, groups, digests, cap, cap_height):
        self._engine = engine
        self._groups = groups        # device buffers [W_j][2^h_j]
        self._digests_dev = digests  # device [nd][4]
        self._digests = None
        self.cap = MerkleCap(cap)
        self.cap_height = cap_height
        self.leaf_heights = [int(g.shape[1]).bit_length() - 1 for g in groups]

    @classmethod
    def new(cls, leaves, cap_height, engine=None):  # batch_merkle_tree.rs:35-130
        """leaves: a list of [2^h_j][W_j] matrices (host), heights strictly decreasing"""
        eng = engine or default_engine()
        host = [np.asarray(m, dtype=np.uint64) for m in leaves]
        if not host or any(m.ndim != 2 for m in host):
            raise ValueError("leaves must be a non-empty list of [rows][w] matrices")  # :36
        for m in host:
            if m.shape[0] != 1 << (int(m.shape[0]).bit_length() - 1):
                raise ValueError("every matrix height must be a power of two")  # :37
        groups = [eng.dev(np.ascontiguousarray(m.T)) for m in host]
        return cls.from_device(groups, cap_height, eng)

    @classmethod
    def from_device(cls, groups, cap_height, engine=None):
        """groups: device buffers [W_j][2^h_j] (column-major matrices), tallest first"""
        eng = engine or default_engine()
        ptrs, strides, widths, logs = _tables(eng, groups)
        nd = eng.num_digests(logs[0], cap_height) if cap_height <= logs[0] else 0
        digests = eng.mem.zeros(max(nd, 1), 4)
        cap = eng.mem.zeros(1 << cap_height, 4)
        eng.check(eng.lib.p2hot_batch_merkle_dev(eng.ctx, ptrs, strides, widths, logs, len(groups), cap_height, eng.ptr(digests),
                                                 eng.ptr(cap)))
        return cls(eng, groups, digests[:nd], eng.host(cap), cap_height)

    @property
    def digests(self):
        if self._digests is None:
            self._digests = self._engine.host(self._digests_dev).reshape(-1, 4)
        return self._digests

    @property
    def leaves(self):
        return [np.ascontiguousarray(self._engine.host(g).T) for g in self._groups]

    def _idx(self, leaf_indices):
        idx = np.ascontiguousarray(np.asarray(leaf_indices, dtype=np.uint64).reshape(-1))
        if idx.size and int(idx.max()) >> self.leaf_heights[0]:
            raise IndexError("leaf index %d out of range (2^%d leaves)" % (int(idx.max()), self.leaf_heights[0]))
        return idx

    def values_many(self, leaf_indices):
        """values(i) flattened for every index: [m][sum_j W_j]"""
        eng, idx = self._engine, self._idx(leaf_indices)
        ptrs, strides, widths, logs = _tables(eng, self._groups)
        total = sum(g.shape[0] for g in self._groups)
        out = eng.mem.zeros(max(len(idx), 1), max(total, 1))
        d_idx = eng.dev(idx if idx.size else np.zeros(1, dtype=np.uint64))
        eng.check(eng.lib.p2hot_batch_merkle_rows_dev(eng.ctx, ptrs, strides, widths, logs, len(self._groups), eng.ptr(d_idx), len(idx),
                                                      eng.ptr(out)))
        return eng.host(out)[:len(idx), :total]

    def values(self, leaf_index):  # :155-164
        row, out, w0 = self.values_many([leaf_index])[0], [], 0
        for g in self._groups:
            out.append(row[w0:w0 + g.shape[0]])
            w0 += g.shape[0]
        return out

    def open_batch_many(self, leaf_indices):
        """[m][h_0 - cap_height][4]"""
        eng, idx = self._engine, self._idx(leaf_indices)
        layers = self.leaf_heights[0] - self.cap_height
        logs = (C.c_uint * len(self.leaf_heights))(*self.leaf_heights)
        out = eng.mem.zeros(max(len(idx), 1), max(layers, 1), 4)
        d_idx = eng.dev(idx if idx.size else np.zeros(1, dtype=np.uint64))
        eng.check(eng.lib.p2hot_batch_merkle_paths_dev(eng.ctx, eng.ptr(self._digests_dev), logs, len(self.leaf_heights), self.cap_height,
                                                       eng.ptr(d_idx), len(idx), eng.ptr(out)))
        return eng.host(out)[:len(idx), :layers]

    def open_batch(self, leaf_index):  # :133-153
        return self.open_batch_many([leaf_index])[0]
