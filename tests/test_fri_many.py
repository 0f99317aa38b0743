"""The opening proofs of M proofs per set of launches: p2hot_fri_commit_many_dev, p2hot_fri_pow_many and the fused path of
p2hot_prove_openings_many against M calls of p2hot_fri_commit_dev / p2hot_fri_pow / p2hot_prove_openings, word for word, the
transcripts afterwards included (three challenges drawn from each).
Proof j's transcript has observed 5 + j elements before the call, so the input buffers hold different counts and, from j = 3 on, a
transcript crosses the duplex at 8 inputs on its own."""
import ctypes as C

import numpy as np
import pytest

from plonky2_amd import _lib
from tests.conftest import P, rand_field

BASE = (6, 3, 2, [2, 1], 0, 0)  # log_n, rate_bits, cap_height, arity bits, max_num_query_steps, final_poly_coeff_len


def _sizes(log_n, rb, cap, arity):
    """words per proof of the round leaves and digests, and the final polynomial's length"""
    m, leaf_words, dig_words = 1 << (log_n + rb), 0, 0
    for ab in arity:
        leaf_words += 2 * m
        dig_words += 4 * max(0, 2 * ((m >> ab) - (1 << cap)))
        m >>= ab
    return leaf_words, dig_words, m >> rb


def _challengers(eng, M):
    from plonky2_amd.iop.challenger import Challenger
    chs = [Challenger(eng) for _ in range(M)]
    for j, ch in enumerate(chs):
        ch.observe_elements(np.arange(100 + j, 105 + 2 * j, dtype=np.uint64))  # 5 + j elements
    return chs


def _commit(eng, planes, shape, many, digests_on_device=True):
    """planes: host [2][M][n].  Returns proof-major (leaves, digests, caps, betas, final, transcript draws)"""
    log_n, rb, cap, arity, mqs, fpl = shape
    M, n, R = planes.shape[1], 1 << log_n, len(arity)
    leaf_words, dig_words, n_final = _sizes(log_n, rb, cap, arity)
    ab = (C.c_uint * max(1, R))(*arity)
    chs = _challengers(eng, M)
    d_leaves = eng.mem.zeros(M, max(1, leaf_words))
    digests = eng.mem.zeros(M, max(1, dig_words)) if digests_on_device else np.zeros((M, max(1, dig_words)), dtype=np.uint64)
    dig_ptr = (lambda a: eng.ptr(a)) if digests_on_device else (lambda a: a.ctypes.data)
    caps = np.zeros((M, max(1, R), 4 << cap), dtype=np.uint64)
    betas = np.zeros((M, max(1, R), 2), dtype=np.uint64)
    final = np.zeros((M, n_final, 2), dtype=np.uint64)
    if many:
        d_planes = eng.dev(planes)
        cp = (C.c_void_p * M)(*[ch._h for ch in chs])
        eng.check(eng.lib.p2hot_fri_commit_many_dev(eng.ctx, M, eng.ptr(d_planes), log_n, rb, cap, ab, R, mqs, fpl, cp, eng.ptr(d_leaves),
                                                    dig_ptr(digests), int(digests_on_device), caps.ctypes.data, betas.ctypes.data,
                                                    final.ctypes.data))
    else:
        for j in range(M):
            d_planes = eng.dev(np.ascontiguousarray(planes[:, j]))
            eng.check(eng.lib.p2hot_fri_commit_dev(eng.ctx, eng.ptr(d_planes), log_n, rb, cap, ab, R, mqs, fpl, chs[j]._h, eng.ptr(d_leaves[j]),
                                                   dig_ptr(digests[j]), int(digests_on_device), caps[j].ctypes.data, betas[j].ctypes.data,
                                                   final[j].ctypes.data))
    return (eng.host(d_leaves), eng.host(digests) if digests_on_device else digests, caps, betas, final,
            [ch.get_n_challenges(3) for ch in chs])


def _assert_same_commit(a, b, M):
    for k, name in enumerate(("leaves", "digests", "caps", "betas", "final")):
        for j in range(M):
            assert (np.asarray(a[k][j]) == np.asarray(b[k][j])).all(), (name, j)
    assert a[5] == b[5]  # the transcripts afterwards
    assert len({tuple(t) for t in b[5]}) == M  # M different transcripts


def test_the_two_symbols_exist_and_are_bound(eng):
    for name in ("p2hot_fri_commit_many_dev", "p2hot_fri_pow_many"):
        assert name in _lib.SIGNATURES and getattr(eng.lib, name).argtypes == _lib.SIGNATURES[name][1]


@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_fri_commit_many_equals_single_calls(eng, M):
    """the base shape; M = 3 is no power of two (a forest of 3 << cap_height cap subtrees), at M = 8 proofs 3.. cross the duplex"""
    rng = np.random.default_rng(700 + M)
    planes = rand_field(rng, 2, M, 1 << BASE[0], noncanonical=True)
    _assert_same_commit(_commit(eng, planes, BASE, False), _commit(eng, planes, BASE, True), M)


@pytest.mark.parametrize("shape", [
    (6, 3, 2, [], 0, 0),        # n_reduction_rounds = 0: only the final polynomial is observed
    (2, 1, 2, [1], 0, 0),       # the round tree is all cap: 4 leaves, cap height 2, no digests
    (6, 3, 2, [2, 1], 4, 24),   # max_num_query_steps above the rounds, final_poly_coeff_len above the final length (8)
    (2, 1, 1, [1], 3, 40),      # ... with more zero padding (76 words) than one observation launch takes (2 N = 16)
    (5, 3, 2, [3], 0, 0),       # log_n = 5, arity 8
], ids=["no_rounds", "all_cap", "padding", "padding_chunks", "arity8"])
def test_fri_commit_many_degenerate_geometry(eng, shape):
    M = 3
    rng = np.random.default_rng(710)
    planes = rand_field(rng, 2, M, 1 << shape[0])
    _assert_same_commit(_commit(eng, planes, shape, False), _commit(eng, planes, shape, True), M)


def test_fri_commit_many_host_digests(eng):
    M = 3
    planes = rand_field(np.random.default_rng(711), 2, M, 1 << BASE[0])
    _assert_same_commit(_commit(eng, planes, BASE, False, digests_on_device=False), _commit(eng, planes, BASE, True, digests_on_device=False), M)


def test_fri_commit_many_two_groups(eng, monkeypatch):
    """P2HOT_MANY_GROUP lowers the proofs per group: M = 3 runs as a group of two and a group of one"""
    M = 3
    planes = rand_field(np.random.default_rng(712), 2, M, 1 << BASE[0])
    monkeypatch.delenv("P2HOT_MANY_GROUP", raising=False)
    one = _commit(eng, planes, BASE, True)
    monkeypatch.setenv("P2HOT_MANY_GROUP", "2")
    two = _commit(eng, planes, BASE, True)
    monkeypatch.delenv("P2HOT_MANY_GROUP")
    _assert_same_commit(_commit(eng, planes, BASE, False), two, M)
    _assert_same_commit(one, two, M)


def _pow(eng, M, pow_bits, many):
    chs = _challengers(eng, M)
    w = (C.c_uint64 * M)()
    if many:
        cp = (C.c_void_p * M)(*[ch._h for ch in chs])
        eng.check(eng.lib.p2hot_fri_pow_many(eng.ctx, M, cp, pow_bits, w))
    else:
        for j in range(M):
            one = C.c_uint64()
            eng.check(eng.lib.p2hot_fri_pow(eng.ctx, chs[j]._h, pow_bits, C.byref(one)))
            w[j] = one.value
    return [int(x) for x in w], [ch.get_n_challenges(3) for ch in chs]


@pytest.mark.parametrize("M", [1, 3, 8])
def test_fri_pow_many_equals_single_calls(eng, M):
    assert _pow(eng, M, 3, False) == _pow(eng, M, 3, True)


def test_fri_pow_many_witnesses_in_different_blocks(eng):
    """pow_bits = 8: the smallest witnesses of the 8 transcripts differ and fall into different 256-candidate blocks of the grid
    (blockIdx.x), so blocks of one proof retire or run independently of the other proofs' in the same launch"""
    single = _pow(eng, 8, 8, False)
    assert len(set(single[0])) >= 4 and len({w >> 8 for w in single[0]}) >= 2, single[0]
    assert single == _pow(eng, 8, 8, True)


def test_fri_pow_many_one_proof_misses_the_device_range(eng, monkeypatch):
    """P2HOT_POW_RANGE_LOG = -pow_bits: the device-searched range is the single candidate 0.  Of these 8 transcripts some have the
    witness 0 (a hit) and the others miss and continue alone with host-checked chunks, inside the same call"""
    monkeypatch.setenv("P2HOT_POW_RANGE_LOG", "-2")
    single = _pow(eng, 8, 2, False)
    assert any(w == 0 for w in single[0]) and any(w != 0 for w in single[0]), single[0]
    assert single == _pow(eng, 8, 2, True)


def test_fri_many_errors_come_before_any_work(eng):
    """a refused call names the proof and leaves every transcript as it was"""
    from plonky2_amd.engine import Engine
    from plonky2_amd.iop.challenger import Challenger
    log_n, rb, cap, arity, _, _ = BASE
    M = 3
    chs = _challengers(eng, M)
    before = [ch.compact() for ch in chs]
    d_planes = eng.dev(rand_field(np.random.default_rng(713), 2, M, 1 << log_n))
    ab = (C.c_uint * 2)(*arity)
    w = (C.c_uint64 * M)()

    def commit(cp, planes=d_planes, arity_bits=ab, n_rounds=2):
        return eng.lib.p2hot_fri_commit_many_dev(eng.ctx, M, eng.ptr(planes) if planes is not None else None, log_n, rb, cap, arity_bits,
                                                 n_rounds, 0, 0, cp, None, None, 1, None, None, None)

    def err():
        return eng.lib.p2hot_last_error(eng.ctx).decode()

    good = [ch._h for ch in chs]
    # a null transcript of proof 1
    cp = (C.c_void_p * M)(good[0], None, good[2])
    assert commit(cp) == _lib.EINVAL and "challenger 1" in err()
    assert eng.lib.p2hot_fri_pow_many(eng.ctx, M, cp, 3, w) == _lib.EINVAL and "challenger 1" in err()
    # a transcript of another context
    other = Engine(0, lib=eng.lib, memory=eng.mem)
    foreign = Challenger(other)
    cp = (C.c_void_p * M)(good[0], good[1], foreign._h)
    assert commit(cp) == _lib.EINVAL and "challenger 2" in err()
    assert eng.lib.p2hot_fri_pow_many(eng.ctx, M, cp, 3, w) == _lib.EINVAL and "challenger 2" in err()
    # the same transcript twice
    cp = (C.c_void_p * M)(good[0], good[1], good[0])
    assert commit(cp) == _lib.EINVAL and "challenger 2" in err()
    # a Keccak transcript
    k = C.c_void_p()
    eng.check(eng.lib.p2hot_challenger_create_keccak(eng.ctx, 25, C.byref(k)))
    cp = (C.c_void_p * M)(k, good[1], good[2])
    assert commit(cp) == _lib.EUNSUPPORTED and "challenger 0" in err()
    assert eng.lib.p2hot_fri_pow_many(eng.ctx, M, cp, 3, w) == _lib.EUNSUPPORTED and "challenger 0" in err()
    eng.lib.p2hot_challenger_destroy(k)
    # null planes, a null schedule, a schedule whose second round has fewer leaves than the cap, a grind of more than 64 bits
    cp = (C.c_void_p * M)(*good)
    assert commit(cp, planes=None) == _lib.EINVAL
    assert commit(cp, arity_bits=None) == _lib.EINVAL
    bad = (C.c_uint * 2)(3, 5)
    assert commit(cp, arity_bits=bad) == _lib.EINVAL
    assert eng.lib.p2hot_fri_pow_many(eng.ctx, M, cp, 65, w) == _lib.EINVAL
    assert eng.lib.p2hot_fri_pow_many(eng.ctx, M, cp, 3, None) == _lib.EINVAL
    assert [ch.compact() for ch in chs] == before
    del foreign
    other.close()


# ---------------------------------------------------------------- p2hot_prove_openings_many: the fused path against single calls
PO_BASE = dict(log_n=6, rb=3, cap=2, arity=[2, 1], Q=4, pow_bits=3, mqs=0, fpl=0)
PO_NAMES = ("caps", "final_poly", "initial_leaves", "initial_paths", "step_evals", "step_paths")


class _Case:
    """M proofs of one shape: oracles of widths (5, 3) per proof -- committed separately, or the M oracles of a position by one
    p2hot_commit_many (shared block), or position 1 salted (leaves of 3 + 4 words) -- opened in two batches: every polynomial at
    zeta_j, the first two of oracle 0 at g zeta_j."""

    def __init__(self, eng, M, seed, shared=False, salted=False, same_point=False, widths=(5, 3), **shape):
        from plonky2_amd.fri.oracle import PolynomialBatch
        self.eng, self.M, self.widths = eng, M, list(widths)
        self.p = dict(PO_BASE, **shape)
        log_n, rb, cap = self.p["log_n"], self.p["rb"], self.p["cap"]
        rng = np.random.default_rng(seed)
        n = 1 << log_n
        self.coeffs = [[rand_field(rng, w, n) for w in widths] for _ in range(M)]
        if shared:
            Mp = 1 << (M - 1).bit_length()  # p2hot_commit_many takes a power of two: the spare proofs' oracles stay unused
            per_pos = [PolynomialBatch.from_coeffs_many(np.stack([self.coeffs[j % M][o] for j in range(Mp)]), rb, cap, engine=eng)
                       for o in range(len(widths))]
            self.oracles = [[per_pos[o][j] for o in range(len(widths))] for j in range(M)]
        else:
            self.oracles = [[PolynomialBatch.from_coeffs(self.coeffs[j][o], rb, salted and o == 1, cap, engine=eng,
                                                         salts=rand_field(rng, 4, n << rb) if salted and o == 1 else None)
                             for o in range(len(widths))] for j in range(M)]
        self.leaf_widths = [w + (4 if salted and o == 1 else 0) for o, w in enumerate(widths)]
        g = pow(7, (P - 1) >> log_n, P) if log_n else 1  # any fixed element: the second point only has to differ from the first
        zs = [[int(x) for x in rand_field(rng, 2)] for _ in range(M)]
        if same_point:
            zs = [zs[0]] * M
        self.points = [[z, [z[0] * g % P, z[1] * g % P]] for z in zs]
        self.polys = [[(o, i) for o, w in enumerate(widths) for i in range(w)], [(0, 0), (0, 1)]]
        ab = (C.c_uint * max(1, len(self.p["arity"])))(*self.p["arity"])
        self.fp = _lib.FriParams(rb, cap, self.p["pow_bits"], self.p["Q"], ab, len(self.p["arity"]), 0, self.p["mqs"], self.p["fpl"])
        self.lay = _lib.FriProofLayout()
        h0 = (C.c_void_p * len(widths))(*[o._h for o in self.oracles[0]])
        assert eng.lib.p2hot_fri_proof_sizes(h0, len(widths), C.byref(self.fp), C.byref(self.lay)) == _lib.OK

    def infos(self, j, polys=None):
        from plonky2_amd.fri.oracle import fri_batch_infos
        keep = []
        inf = fri_batch_infos(list(zip(self.points[j], polys or self.polys)), keep)
        return inf, keep

    def run(self, many, polys_of=None, null_buffer_of=None, challengers=None):
        """-> (rc, buffers [M], query indices [M], witnesses [M], transcripts afterwards [M]).  polys_of: {proof: its own lists}"""
        eng, M, Q = self.eng, self.M, self.p["Q"]
        chs = challengers or _challengers(eng, M)
        bufs = [{k: np.zeros(max(1, getattr(self.lay, k + "_words")), dtype=np.uint64) for k in PO_NAMES} for _ in range(M)]
        qidx = [np.zeros(max(1, Q), dtype=np.uint64) for _ in range(M)]
        infos = [self.infos(j, (polys_of or {}).get(j)) for j in range(M)]
        proofs = (_lib.FriProof * M)()
        for j in range(M):
            b = bufs[j]
            proofs[j] = _lib.FriProof(b["caps"].ctypes.data, b["final_poly"].ctypes.data, 0, qidx[j].ctypes.data, b["initial_leaves"].ctypes.data,
                                      b["initial_paths"].ctypes.data, b["step_evals"].ctypes.data, b["step_paths"].ctypes.data)
        if null_buffer_of is not None:
            proofs[null_buffer_of].final_poly = None
        nw = len(self.widths)
        rc = _lib.OK
        if many:
            bp = (C.POINTER(_lib.FriBatchInfo) * M)(*[C.cast(inf, C.POINTER(_lib.FriBatchInfo)) for inf, _ in infos])
            nb = (C.c_size_t * M)(*([2] * M))
            hs = (C.c_void_p * (M * nw))(*[o._h for row in self.oracles for o in row])
            cp = (C.c_void_p * M)(*[ch._h for ch in chs])
            rc = eng.lib.p2hot_prove_openings_many(eng.ctx, M, bp, nb, hs, nw, cp, C.byref(self.fp), proofs)
        else:
            for j in range(M):
                hs = (C.c_void_p * nw)(*[o._h for o in self.oracles[j]])
                eng.check(eng.lib.p2hot_prove_openings(eng.ctx, infos[j][0], 2, hs, nw, chs[j]._h, C.byref(self.fp), C.byref(proofs[j])))
        return rc, bufs, qidx, [int(proofs[j].pow_witness) for j in range(M)], [ch.get_n_challenges(3) for ch in chs]


def _assert_same_proofs(a, b, M, distinct=True):
    assert a[0] == _lib.OK and b[0] == _lib.OK
    for j in range(M):
        for k in PO_NAMES:
            assert (a[1][j][k] == b[1][j][k]).all(), (j, k)
        assert (a[2][j] == b[2][j]).all() and a[3][j] == b[3][j] and a[4][j] == b[4][j], j
    if distinct:
        assert len({tuple(x["final_poly"].tolist()) for x in b[1]}) == M


@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_prove_openings_many_fused_equals_single_calls(eng, monkeypatch, M):
    monkeypatch.delenv("P2HOT_MANY_FUSED", raising=False)
    case = _Case(eng, M, 800 + M)
    _assert_same_proofs(case.run(False), case.run(True), M)


@pytest.mark.parametrize("kind", ["shared_block", "salted", "same_point"])
def test_prove_openings_many_oracle_and_point_variants(eng, monkeypatch, kind):
    """oracles out of one p2hot_commit_many (interleaved columns, strides M N and M n), a salted oracle (leaf width 7, polynomial width
    3), every proof at the same point"""
    monkeypatch.delenv("P2HOT_MANY_FUSED", raising=False)
    M = 4 if kind == "shared_block" else 3
    case = _Case(eng, M, 810, shared=kind == "shared_block", salted=kind == "salted", same_point=kind == "same_point")
    _assert_same_proofs(case.run(False), case.run(True), M)


@pytest.mark.parametrize("shape", [
    dict(arity=[]),                               # n_reduction_rounds = 0
    dict(log_n=2, rb=1, cap=2, arity=[1], Q=3),   # the round tree is all cap (pa_w = 0)
    dict(mqs=4, fpl=24),                          # max_num_query_steps above the rounds, final_poly_coeff_len above the final length
    dict(Q=0),
    dict(log_n=5, arity=[3]),
], ids=["no_rounds", "all_cap", "padding", "no_queries", "arity8"])
def test_prove_openings_many_degenerate_geometry(eng, monkeypatch, shape):
    monkeypatch.delenv("P2HOT_MANY_FUSED", raising=False)
    case = _Case(eng, 3, 820, **shape)
    _assert_same_proofs(case.run(False), case.run(True), 3)


def test_prove_openings_many_two_groups(eng, monkeypatch):
    monkeypatch.delenv("P2HOT_MANY_FUSED", raising=False)
    case = _Case(eng, 3, 830)
    single = case.run(False)
    monkeypatch.setenv("P2HOT_MANY_GROUP", "2")
    two = case.run(True)
    monkeypatch.delenv("P2HOT_MANY_GROUP")
    _assert_same_proofs(single, two, 3)


def test_prove_openings_many_grind_in_different_blocks(eng, monkeypatch):
    monkeypatch.delenv("P2HOT_MANY_FUSED", raising=False)
    case = _Case(eng, 8, 840, pow_bits=8, Q=2)
    single = case.run(False)
    assert len(set(single[3])) >= 4 and len({w >> 8 for w in single[3]}) >= 2, single[3]
    _assert_same_proofs(single, case.run(True), 8)


def test_prove_openings_many_one_proof_misses_the_device_range(eng, monkeypatch):
    """the device range is the single candidate 0: the proofs whose witness is 0 hit, the others are proved again alone from their
    transcripts before the call, inside the same call"""
    monkeypatch.delenv("P2HOT_MANY_FUSED", raising=False)
    monkeypatch.setenv("P2HOT_POW_RANGE_LOG", "-2")
    case = _Case(eng, 8, 852, pow_bits=2, Q=2)  # (the seed: witnesses 1, 0, 10, 1, 4, 7, 0, 2)
    single = case.run(False)
    assert any(w == 0 for w in single[3]) and any(w != 0 for w in single[3]), single[3]
    _assert_same_proofs(single, case.run(True), 8)


def test_prove_openings_many_paths_agree_and_differ_in_when_they_validate(eng, monkeypatch):
    """P2HOT_MANY_FUSED = 0 and = 1 give equal bytes for M = 3.  What tells the paths apart from outside: the fused path validates
    every proof before the first enqueue, the side-by-side path proof by proof -- a null buffer of proof 1 leaves transcript 0
    (and 2) advanced there and every transcript untouched here."""
    case = _Case(eng, 3, 860)
    monkeypatch.setenv("P2HOT_MANY_FUSED", "0")
    side = case.run(True)
    monkeypatch.setenv("P2HOT_MANY_FUSED", "1")
    fused = case.run(True)
    _assert_same_proofs(side, fused, 3)
    fresh = [ch.get_n_challenges(3) for ch in _challengers(eng, 3)]
    monkeypatch.setenv("P2HOT_MANY_FUSED", "0")
    bad = case.run(True, null_buffer_of=1)
    assert bad[0] == _lib.EINVAL and bad[4][0] != fresh[0] and bad[4][1] == fresh[1]
    monkeypatch.setenv("P2HOT_MANY_FUSED", "1")
    bad = case.run(True, null_buffer_of=1)
    assert bad[0] == _lib.EINVAL and "proof 1" in eng.lib.p2hot_last_error(eng.ctx).decode() and bad[4] == fresh


def test_prove_openings_many_heterogeneous_call_falls_back(eng, monkeypatch):
    """proof 1 opens another polynomial list: not one shape, so the call runs side by side and still returns the single calls' bytes"""
    monkeypatch.delenv("P2HOT_MANY_FUSED", raising=False)
    case = _Case(eng, 3, 870)
    other = {1: [case.polys[0][:-1], [(1, 0), (1, 2)]]}
    _assert_same_proofs(case.run(False, polys_of=other), case.run(True, polys_of=other), 3)


def test_a_proof_of_a_fused_call_passes_the_reference_verifier(eng, ora, monkeypatch):
    """M = 4: transcripts that have observed their oracles' caps, points drawn from them, openings observed; proof 2 of the fused
    call verifies under oracle/fri_verifier.py with the oracle's own challenger"""
    from oracle import fri_verifier as fv
    from plonky2_amd.fri.oracle import eval_openings, shape_fri_proof
    from plonky2_amd.iop.challenger import Challenger
    monkeypatch.delenv("P2HOT_MANY_FUSED", raising=False)
    M, k = 4, 2
    case = _Case(eng, M, 880, Q=5)
    p = case.p
    g = ora.root_of_unity(p["log_n"])
    chs, ocs, openings = [], [], []
    for j in range(M):
        c, oc = Challenger(eng), ora.Challenger()
        for ch in (c, oc):
            for o in case.oracles[j]:
                ch.observe_cap(np.asarray(o.merkle_tree.cap.entries))
        zeta = [int(x) for x in c.get_extension_challenge()]
        assert zeta == [int(x) for x in oc.get_extension_challenge()]
        case.points[j] = [zeta, [zeta[0] * g % P, zeta[1] * g % P]]
        ev = eval_openings(case.oracles[j], case.points[j], eng)  # [oracle][point][poly][2]
        op = [[ev[oi][bi][pi] for (oi, pi) in polys] for bi, polys in enumerate(case.polys)]
        for ch in (c, oc):
            for vals in op:
                ch.observe_elements(np.asarray(vals, dtype=np.uint64).reshape(-1))
        chs.append(c), ocs.append(oc), openings.append(op)
    rc, bufs, qidx, wit, _ = case.run(True, challengers=chs)
    assert rc == _lib.OK
    b = dict(bufs[k], final_poly=bufs[k]["final_poly"][:case.lay.final_poly_words])
    proof = shape_fri_proof(b, wit[k], qidx[k], case.leaf_widths, p["log_n"] + p["rb"], p["cap"], p["arity"], p["Q"])
    inst = list(zip(case.points[k], case.polys))
    caps = [np.asarray(o.merkle_tree.cap.entries) for o in case.oracles[k]]
    chal = fv.fri_challenges(ocs[k], proof["commit_phase_merkle_caps"], proof["final_poly"], proof["pow_witness"], p["log_n"], p["rb"], p["cap"], p["Q"])
    fv.verify_fri_proof(inst, openings[k], chal, caps, proof, p["log_n"], p["rb"], p["arity"], p["pow_bits"], p["Q"])


def test_prove_openings_many_errors_come_before_any_work(eng, monkeypatch):
    from plonky2_amd.engine import Engine
    from plonky2_amd.fri.oracle import PolynomialBatch
    from plonky2_amd.iop.challenger import Challenger
    monkeypatch.delenv("P2HOT_MANY_FUSED", raising=False)
    M = 3
    case = _Case(eng, M, 890)
    fresh = [ch.get_n_challenges(3) for ch in _challengers(eng, M)]

    def err():
        return eng.lib.p2hot_last_error(eng.ctx).decode()

    # a null buffer of proof 2
    bad = case.run(True, null_buffer_of=2)
    assert bad[0] == _lib.EINVAL and "proof 2" in err() and bad[4] == fresh
    # an oracle of another degree, rate or cap height in proof 1
    good = case.oracles[1][1]
    rng = np.random.default_rng(891)
    for log_n, rb, cap in ((5, 3, 2), (6, 2, 2), (6, 3, 1)):
        case.oracles[1][1] = PolynomialBatch.from_coeffs(rand_field(rng, 3, 1 << log_n), rb, False, cap, engine=eng)
        bad = case.run(True)
        assert bad[0] == _lib.EINVAL and "proof 1" in err() and bad[4] == fresh, (log_n, rb, cap)
    case.oracles[1][1] = good
    # a transcript of another context; a Keccak transcript
    other = Engine(0, lib=eng.lib, memory=eng.mem)
    chs = _challengers(eng, M)
    foreign = Challenger(other)
    bad = case.run(True, challengers=[chs[0], foreign, chs[2]])
    assert bad[0] == _lib.EINVAL and "challenger 1" in err() and [bad[4][0], bad[4][2]] == [fresh[0], fresh[2]]
    from plonky2_amd.hash.keccak import KeccakHash
    chs = _challengers(eng, M)
    bad = case.run(True, challengers=[chs[0], chs[1], Challenger(eng, hasher=KeccakHash(25))])
    assert bad[0] == _lib.EUNSUPPORTED and bad[4][:2] == fresh[:2]
    del foreign
    other.close()
