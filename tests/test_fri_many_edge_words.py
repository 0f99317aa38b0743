"""The M-forms of the opening proof's arithmetic kernels on edge words (the pattern of tests/test_edge_words.py): one edge proof
between two random ones.  The edge proof's planes / coefficient columns hold the whole edge grid of the field -- 0, 1, P - 1,
2^32 - 1, 2^32, P - 2^32 among it, raw words of [P, 2^64) too -- a different word in every lane, and the results are checked
against Python integers row by row; the transcript kernel runs on edge sponge states against the oracle's permutation."""
import ctypes as C

import numpy as np
import pytest

from plonky2_amd import _lib
from tests import edge_words as ew
from tests.conftest import P, rand_field
from tests.pyref import ext_add, ext_mul

E32 = 2**32
EDGE = [0, 1, P - 1, E32 - 1, E32, P - E32]
M = 3


def _transcripts(eng, ora):
    """device transcripts and their oracle twins after 5 + j observed elements"""
    from plonky2_amd.iop.challenger import Challenger
    chs, ocs = [Challenger(eng) for _ in range(M)], [ora.Challenger() for _ in range(M)]
    for j in range(M):
        for c in (chs[j], ocs[j]):
            c.observe_elements(np.arange(40 + j, 45 + 2 * j, dtype=np.uint64))
    return chs, ocs


def _fold(coeffs, beta, ab):
    """coeffs'[j] = sum_i beta^i coeffs[(j << ab) + i] (plonk_common.rs:120-132)"""
    out = []
    for j in range(len(coeffs) >> ab):
        acc = (0, 0)
        for i in reversed(range(1 << ab)):
            acc = ext_add(ext_mul(acc, beta), coeffs[(j << ab) + i])
        out.append(acc)
    return out


@pytest.mark.parametrize("arity", [[1], [2], [3], [2, 1]], ids=lambda a: "arity" + "_".join(map(str, a)))
def test_fold_many_on_edge_planes(eng, ora, arity):
    """fri::fold_many_kernel through p2hot_fri_commit_many_dev: the final polynomials are the planes folded by the betas the call
    returns (checked against the single calls and the oracle elsewhere), every row against Python integers"""
    log_n, rb, cap = 6, 1, 0
    n, R = 1 << log_n, len(arity)
    rng = np.random.default_rng(9100 + sum(arity))
    planes = rand_field(rng, 2, M, n)
    planes[:, 1, :] = ew.edge_matrix(rng, 2, n, canonical=False)
    assert set(EDGE) <= set(int(v) for v in planes[0, 1]) and set(EDGE) <= set(int(v) for v in planes[1, 1])
    chs, _ = _transcripts(eng, ora)
    betas = np.zeros((M, R, 2), dtype=np.uint64)
    final = np.zeros((M, n >> sum(arity), 2), dtype=np.uint64)
    ab = (C.c_uint * R)(*arity)
    cp = (C.c_void_p * M)(*[c._h for c in chs])
    d_planes = eng.dev(planes)
    eng.check(eng.lib.p2hot_fri_commit_many_dev(eng.ctx, M, eng.ptr(d_planes), log_n, rb, cap, ab, R, 0, 0, cp, None, None, 1, None,
                                                betas.ctypes.data, final.ctypes.data))
    for j in range(M):
        co = [(int(planes[0, j, t]) % P, int(planes[1, j, t]) % P) for t in range(n)]
        for r, a in enumerate(arity):
            co = _fold(co, (int(betas[j, r, 0]), int(betas[j, r, 1])), a)
        for t, want in enumerate(co):
            assert (int(final[j, t, 0]), int(final[j, t, 1])) == want, (j, t)


def _final_poly_ref(cols, batches, alpha):
    """oracle.rs:190-213 in Python integers: cols[oracle][poly][t]; batches [(z, [(oracle, poly)..])..]"""
    n = len(cols[0][0])
    final = [(0, 0)] * n
    for z, polys in batches:
        apow, comp = (1, 0), [(0, 0)] * n
        for (o, i) in polys:  # reduce_polys_base (reducing.rs:83-95)
            comp = [ext_add(comp[t], (apow[0] * (int(cols[o][i][t]) % P) % P, apow[1] * (int(cols[o][i][t]) % P) % P)) for t in range(n)]
            apow = ext_mul(apow, alpha)
        b, quo = (0, 0), [(0, 0)] * n  # divide_by_linear (division.rs:79-92), padded with a zero
        for k in reversed(range(n)):
            b = ext_add(ext_mul(b, z), comp[k])
            if k >= 1:
                quo[k - 1] = b
        final = [ext_add(ext_mul(final[t], apow), quo[t]) for t in range(n)]  # shift_poly + add (reducing.rs:103-106)
    return final


def _final_polys(eng, ora, log_n, seed, check_ints):
    """prove_openings_many with no reduction rounds and no queries: final_poly IS the final polynomial of the prelude"""
    widths, rb, cap = [2, 3], 1, 0
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    cols = [[rand_field(rng, w, n) for w in widths] for _ in range(M)]
    rows = min(n, 4096)
    cols[1] = [np.tile(ew.edge_matrix(rng, w, rows, canonical=False), n // rows) for w in widths]
    oracles = [[ew.wrap(eng, np.zeros((w, n << rb), dtype=np.uint64), log_n, rb, cap, coeffs=cols[j][o]) for o, w in enumerate(widths)] for j in range(M)]
    points = [[[int(x) for x in rand_field(rng, 2)] for _ in range(2)] for _ in range(M)]
    points[1] = [[P - 1, E32], [E32 - 1, P - E32]]
    polys = [[(o, i) for o, w in enumerate(widths) for i in range(w)], [(0, 0), (0, 1)]]
    from plonky2_amd.fri.oracle import fri_batch_infos
    ab = (C.c_uint * 1)()
    fp = _lib.FriParams(rb, cap, 0, 0, ab, 0, 0, 0, 0)

    def run(many):
        chs, ocs = _transcripts(eng, ora)
        final = [np.zeros(2 * n, dtype=np.uint64) for _ in range(M)]
        one = np.zeros(1, dtype=np.uint64)
        proofs = (_lib.FriProof * M)(*[_lib.FriProof(one.ctypes.data, final[j].ctypes.data, 0, None, None, None, None, None) for j in range(M)])
        keep, infos = [], []
        for j in range(M):
            infos.append(fri_batch_infos(list(zip(points[j], polys)), keep))
        if many:
            bp = (C.POINTER(_lib.FriBatchInfo) * M)(*[C.cast(inf, C.POINTER(_lib.FriBatchInfo)) for inf in infos])
            nb = (C.c_size_t * M)(*([2] * M))
            hs = (C.c_void_p * (M * 2))(*[o._h for row in oracles for o in row])
            cp = (C.c_void_p * M)(*[c._h for c in chs])
            eng.check(eng.lib.p2hot_prove_openings_many(eng.ctx, M, bp, nb, hs, 2, cp, C.byref(fp), proofs))
        else:
            for j in range(M):
                hs = (C.c_void_p * 2)(*[o._h for o in oracles[j]])
                eng.check(eng.lib.p2hot_prove_openings(eng.ctx, infos[j], 2, hs, 2, chs[j]._h, C.byref(fp), C.byref(proofs[j])))
        return final, ocs

    final, ocs = run(True)
    single, _ = run(False)
    for j in range(M):
        assert (final[j] == single[j]).all(), j
    if check_ints:
        for j in range(M):
            alpha = tuple(int(x) for x in ocs[j].get_extension_challenge())
            want = _final_poly_ref(cols[j], [(tuple(z), p) for z, p in zip(points[j], polys)], alpha)
            got = final[j].reshape(n, 2)
            for t in range(n):
                assert (int(got[t, 0]), int(got[t, 1])) == want[t], (j, t)


def test_final_poly_many_on_edge_coefficients(eng, ora, monkeypatch):
    """alpha_powers, reduce_polys_base_small and the chunk-total, carry and emit kernels in M-form, every row against Python integers"""
    monkeypatch.delenv("P2HOT_MANY_FUSED", raising=False)
    _final_polys(eng, ora, 6, 9200, True)


def test_final_poly_many_two_level_carries_on_edge_coefficients(eng, ora, monkeypatch):
    """past the two-level switch of the carry scan (horner_group_walk in M-form), on a context with a lowered P2HOT_HORNER_2L_MIN:
    2^10 coefficients are 256 chunks in 4 groups.  Word for word against the single calls of the same context, which
    tests/test_edge_words.py holds to the oracle past that switch"""
    from plonky2_amd.engine import Engine
    monkeypatch.delenv("P2HOT_MANY_FUSED", raising=False)
    monkeypatch.setenv("P2HOT_HORNER_2L_MIN", "16")
    e = Engine(0, lib=eng.lib, memory=eng.mem)
    monkeypatch.delenv("P2HOT_HORNER_2L_MIN")
    try:
        _final_polys(e, ora, 10, 9300, False)
    finally:
        e.close()


def test_challenger_many_on_edge_states(eng, ora):
    """fri::challenger_many_kernel on sponge states, input and output buffers made of the edge words, the three transcripts with 3, 7
    and 0 buffered inputs: four elements observed (the second transcript crosses the duplex), the grind's witness observed and
    its response drawn, then three challenges -- against the same steps through the oracle's permutation"""
    from plonky2_amd.iop.challenger import Challenger
    rng = np.random.default_rng(9400)
    chs, ocs = [], []
    for j, (n_in, n_out) in enumerate([(3, 0), (7, 0), (0, 5)]):
        words = [EDGE[int(k)] for k in rng.permutation(28) % len(EDGE)]
        st = _lib.ChallengerState()
        oc = ora.Challenger()
        for i in range(12):
            st.sponge_state[i] = oc.s.state[i] = words[i]
        for i in range(8):
            st.input_buffer[i] = oc.s.inb[i] = words[12 + i]
            st.output_buffer[i] = oc.s.outb[i] = words[20 + i]
        st.input_len = oc.s.n_in = n_in
        st.output_len = oc.s.n_out = n_out
        c = Challenger(eng)
        c.load_state(st)
        chs.append(c), ocs.append(oc)
    planes = np.zeros((2, M, 2), dtype=np.uint64)
    planes[:, 1, :] = [[P - 1, E32], [E32 - 1, P - E32]]
    planes[:, 2, :] = rand_field(rng, 2, 2)
    cp = (C.c_void_p * M)(*[c._h for c in chs])
    ab = (C.c_uint * 1)()
    final = np.zeros((M, 2, 2), dtype=np.uint64)
    d_planes = eng.dev(planes)
    eng.check(eng.lib.p2hot_fri_commit_many_dev(eng.ctx, M, eng.ptr(d_planes), 1, 1, 0, ab, 0, 0, 0, cp, None, None, 1, None, None, final.ctypes.data))
    w = (C.c_uint64 * M)()
    eng.check(eng.lib.p2hot_fri_pow_many(eng.ctx, M, cp, 0, w))
    for j in range(M):
        assert (final[j] == planes[:, j, :].T % np.uint64(P)).all()
        ocs[j].observe_elements(final[j].reshape(-1))
        assert ora.fri_pow(ocs[j], 0) == int(w[j]) == 0
        assert chs[j].get_n_challenges(3) == ocs[j].get_n_challenges(3), j
        st = chs[j].state()
        assert list(st.sponge_state) == list(ocs[j].s.state) and st.input_len == ocs[j].s.n_in and st.output_len == ocs[j].s.n_out, j
