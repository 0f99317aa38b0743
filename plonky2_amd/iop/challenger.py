"""Challenger -- mirror of plonky2/src/iop/challenger.rs:16-153 over a device-resident sponge.

The duplex sponge state lives on the GPU (libp2hot `p2hot_challenger`), so the FRI commit phase can
observe caps and draw betas without a host round trip; this class is the host handle with the
reference's method names.
"""
import ctypes as C

import numpy as np

from .. import _lib
from ..engine import default_engine


class Challenger:
    def __init__(self, engine=None, hasher=None):  # Challenger::<F, H>::new, challenger.rs:30-37
        """hasher: None = PoseidonHash, or a plonky2_amd.hash.keccak.KeccakHash (the transcript of KeccakGoldilocksConfig)"""
        from ..hash.keccak import hash_size
        self.engine = engine or default_engine()
        self.hasher = hasher
        self._hash_n = hash_size(hasher)
        h = C.c_void_p()
        if self._hash_n:
            self.engine.check(self.engine.lib.p2hot_challenger_create_keccak(self.engine.ctx, self._hash_n, C.byref(h)))
        else:
            self.engine.check(self.engine.lib.p2hot_challenger_create(self.engine.ctx, C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if self._h and self.engine.ctx:
                self.engine.lib.p2hot_challenger_destroy(self._h)
            self._h = None
        except Exception:
            pass

    def _step(self, observe, n_get):
        lib = self.engine.lib
        obs = np.ascontiguousarray(np.asarray(observe, dtype=np.uint64).reshape(-1))
        out = np.zeros(max(n_get, 1), dtype=np.uint64)
        self.engine.check(lib.p2hot_challenger_step(self._h, obs.ctypes.data if obs.size else None, obs.size,
                                                    out.ctypes.data, n_get))
        return [int(x) for x in out[:n_get]]

    # challenger.rs:39-80
    def observe_element(self, e):
        self._step([e], 0)

    def observe_elements(self, es):
        self._step(es, 0)

    def observe_extension_element(self, e):  # to_basefield_array order
        self._step(list(e), 0)

    def observe_extension_elements(self, es):
        self._step(np.asarray(es, dtype=np.uint64).reshape(-1), 0)

    def _observe_digests(self, d):
        """digests of a Keccak transcript: uint8 [count][N] bytes (BytesHash<N>), or their slot words [count][4]"""
        from ..hash.keccak import from_bytes
        d = np.asarray(d)
        if d.dtype == np.uint8:
            if d.shape[-1] != self._hash_n:
                raise ValueError("digests of %d bytes for a KeccakHash<%d> challenger" % (d.shape[-1], self._hash_n))
            slots = from_bytes(d)
        else:
            slots = np.asarray(d, dtype=np.uint64).reshape(-1, 4)
        slots = np.ascontiguousarray(slots)
        if len(slots):
            self.engine.check(self.engine.lib.p2hot_challenger_observe_digests(self._h, slots.ctypes.data, len(slots)))

    def observe_hash(self, h):
        if self._hash_n:
            return self._observe_digests(h)
        self._step(h, 0)

    def observe_cap(self, cap):
        if self._hash_n:
            return self._observe_digests(cap)
        self._step(np.asarray(cap, dtype=np.uint64).reshape(-1), 0)

    # challenger.rs:82-116
    def get_challenge(self):
        return self._step([], 1)[0]

    def get_n_challenges(self, n):
        return self._step([], n)

    def get_hash(self):
        return self.get_n_challenges(4)

    def get_extension_challenge(self):
        return self.get_n_challenges(2)

    def get_n_extension_challenges(self, n):
        return [self.get_extension_challenge() for _ in range(n)]

    # state transfer (what the Rust shim does with sponge_state / input_buffer / output_buffer)
    def state(self):
        st = _lib.ChallengerState()
        self.engine.check(self.engine.lib.p2hot_challenger_store(self._h, C.byref(st)))
        return st

    def load_state(self, st):
        self.engine.check(self.engine.lib.p2hot_challenger_load(self._h, C.byref(st)))

    def compact(self):
        """(sponge_state, input_buffer, output_buffer) as python lists"""
        st = self.state()
        return (list(st.sponge_state), list(st.input_buffer)[:st.input_len], list(st.output_buffer)[:st.output_len])
