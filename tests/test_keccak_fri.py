"""Opening proofs of KeccakGoldilocksConfig on the device: KeccakPermutation, the Keccak challenger, the FRI round trees, the
grind and the whole p2hot_prove_openings, each against tests/keccak_fri_ref.py (the Rust sources restated over tests/keccak_ref.py),
on the emulator (CPU tier) and on the MI355X (-m gpu)."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from plonky2_amd import _lib
from tests import keccak_fri_ref as kf
from tests import keccak_ref as kr
from tests.conftest import P, rand_field

# [c, 0, ..., 0] whose hash onion holds a word >= p among the first twelve (found by a CPU search over c with the reference:
# about one state in 3 * 10^8): (c, index of the rejected stream word, the word, kept words 0 and 1, kept word 7)
REJECTION_STATES = [(398933008, 4, 0xFFFFFFFF60440266, (11907418681015339862, 5231559121053982289), 8837479586456409741),
                    (494183523, 1, 0xFFFFFFFF9072FF53, (557964209534106482, 8800958619029275255), 13982104793188786474)]


def _khash(eng, n):
    from plonky2_amd.hash.keccak import KeccakHash
    return KeccakHash(n, engine=eng)


def _challenger(eng, n=25):
    from plonky2_amd.iop.challenger import Challenger
    return Challenger(eng, hasher=_khash(eng, n))


def _load(ch, sponge_state, input_buffer=(), output_buffer=()):
    st = _lib.ChallengerState()
    for i, v in enumerate(sponge_state):
        st.sponge_state[i] = int(v)
    for i, v in enumerate(input_buffer):
        st.input_buffer[i] = int(v)
    for i, v in enumerate(output_buffer):
        st.output_buffer[i] = int(v)
    st.input_len, st.output_len = len(input_buffer), len(output_buffer)
    ch.load_state(st)


def _ref_at(sponge_state, input_buffer=(), output_buffer=()):
    r = kf.Challenger()
    r.sponge_state = [int(v) for v in sponge_state]
    r.input_buffer = [int(v) for v in input_buffer]
    r.output_buffer = [int(v) for v in output_buffer]
    return r


def _same(ch, ref):
    got, want = ch.compact(), ref.snapshot()
    assert got == tuple(want), (got, want)


# ---------------------------------------------------------------- 1. the permutation
def test_permutation_vs_reference(eng):
    rng = np.random.default_rng(63)
    states = rand_field(rng, 67, 12, noncanonical=True)  # not a multiple of 64
    states[0] = 0
    states[3, 5] = np.uint64(P + 5)
    states[4] = np.uint64(2**64 - 1)
    for k, (c, _, _, _, _) in enumerate(REJECTION_STATES):
        states[1 + k] = 0
        states[1 + k, 0] = c
    # the fixtures, by the reference alone: these two states do reject a word, so a fourth hash is needed
    for k, (c, at, word, first, w7) in enumerate(REJECTION_STATES):
        stream = kf.hash_stream(states[1 + k], 4)
        assert stream[at] == word and word >= P and all(w < P for i, w in enumerate(stream[:13]) if i != at)
        kept = [w for w in stream if w < P][:12]
        assert tuple(kept[:2]) == first and kept[7] == w7 and kept[11] == stream[12]
    ref = kf.permute(states)
    assert (ref < np.uint64(P)).all() and (kf.permute(states % np.uint64(P)) == ref).all()
    for k, (_, _, _, first, w7) in enumerate(REJECTION_STATES):
        assert tuple(int(x) for x in ref[1 + k, :2]) == first and int(ref[1 + k, 7]) == w7
    # the device: a state with empty buffers, 8 challenges = one duplex = one permutation
    ch = _challenger(eng)
    for k in range(len(states)):
        _load(ch, states[k])
        out = ch.get_n_challenges(8)
        want = [int(x) for x in ref[k]]
        assert out == want[7::-1], k              # popped from the back of the rate portion
        assert ch.compact() == (want, [], []), k


# ---------------------------------------------------------------- 2. the challenger
@pytest.mark.parametrize("n", [25, 32])
def test_challenger_vs_reference(eng, n):
    rng = np.random.default_rng(n)
    ch, ref = _challenger(eng, n), kf.Challenger()
    _same(ch, ref)

    def observe(k):
        e = rand_field(rng, k, noncanonical=True)
        ch.observe_elements(e)
        ref.observe_elements(e)

    def draw(k):
        assert ch.get_n_challenges(k) == ref.get_n_challenges(k)

    def digests(k, as_slots):
        d = rng.integers(0, 256, size=(k, n), dtype=np.uint8)
        assert len(kf.bytes_hash_to_vec(d[0])) == {25: 4, 32: 5}[n]
        if as_slots:   # bytes n..32 of a slot are not part of the digest
            s = np.ascontiguousarray(kr.to_slots(d)).view(np.uint8).reshape(k, 32).copy()
            s[:, n:] = 0xA5
            ch.observe_cap(s.view("<u8").astype(np.uint64).reshape(k, 4))
        elif k == 1:
            ch.observe_hash(d[0])
        else:
            ch.observe_cap(d)
        ref.observe_cap(d)

    steps = [(observe, 0), (draw, 1), (observe, 1), (observe, 7), (draw, 8), (observe, 8), (draw, 9), (observe, 9), (draw, 1),
             (observe, 17), (draw, 8), (draw, 1), (digests, 1, False), (draw, 1), (digests, 3, True), (observe, 3), (digests, 4, False),
             (draw, 9), (observe, 7), (observe, 1), (draw, 1)]
    for i, (f, *args) in enumerate(steps):
        f(*args)
        _same(ch, ref)
        if i in (7, 11, 15):   # store -> load in mid-buffer (inputs pending / outputs left), into another handle
            st = ch.state()
            assert 0 < (st.output_len if i == 11 else st.input_len) < 8
            ch = _challenger(eng, n)
            ch.load_state(st)
            _same(ch, ref)


# ---------------------------------------------------------------- 3. the commit phase
def _check_commit(eng, trees, final, betas, ch, o, ref, cap_height, n_hash):
    assert (np.asarray(final) == o["final"]).all() and (np.asarray(betas) == o["betas"]).all()
    assert len(trees) == len(o["caps"])
    for t, lv, d, c in zip(trees, o["leaves"], o["digests"], o["caps"]):
        assert (np.asarray(t.leaves) == lv).all()
        got = np.asarray(eng.host(t.digests) if eng.mem.is_buffer(t.digests) else t.digests, dtype=np.uint64).reshape(-1, 4)
        assert got.shape[0] == len(d) and (got == kr.to_slots(d)).all()
        assert (t.cap.entries == kr.to_slots(c)).all()
        assert t.hasher is ch.hasher
    _same(ch, ref)


FRI_CASES = [  # rate_bits, cap_height, arity_bits, N, max_num_query_steps, final_poly_coeff_len
    (1, 0, [1], 25, None, None),
    (1, 2, [2, 1], 25, None, None),
    (1, 3, [3], 25, None, None),        # the only tree is all cap
    (1, 3, [2, 1], 25, 4, 8),           # the last round's tree is all cap
    (3, 0, [3], 25, None, 8),
    (3, 2, [2, 1], 25, 5, None),
    (3, 2, [1], 32, None, None),        # a leaf of 4 words is copied: hash_or_noop
    (3, 0, [1], 32, 3, 32),             # N > 28: a dummy cap observes 4 zeros per entry, a real one 5 elements
    (1, 2, [2, 1], 32, None, None),
    (3, 2, [3], 32, 2, 8),
]


@pytest.mark.parametrize("rb,cap,arity,n_hash,steps,flen", FRI_CASES)
def test_fri_commit_phase_vs_reference(eng, ora, rb, cap, arity, n_hash, steps, flen):
    from plonky2_amd.fri.prover import fri_committed_trees, fri_committed_trees_device
    rng = np.random.default_rng(rb * 100 + cap * 10 + len(arity) + n_hash)
    log_n = 5
    coeffs = rand_field(rng, 1 << log_n, 2, noncanonical=True)
    pre = rand_field(rng, 3)
    ref = kf.Challenger()
    ref.observe_elements(pre)
    want = ref.clone()
    o = kf.fri_committed_trees(coeffs, want, rb, cap, arity, kr.KeccakHash(n_hash), flen, steps)
    # host pointers
    ch = _challenger(eng, n_hash)
    ch.observe_elements(pre)
    trees, final, betas = fri_committed_trees(coeffs, ch, rb, cap, arity, engine=eng, final_poly_coeff_len=flen,
                                              max_num_query_steps=steps)
    _check_commit(eng, trees, final, betas, ch, o, want, cap, n_hash)
    # device planes in, leaves and digests stay on the device
    ch = _challenger(eng, n_hash)
    ch.observe_elements(pre)
    planes = eng.dev(np.ascontiguousarray(coeffs.T))
    trees, final, betas = fri_committed_trees_device(planes, log_n, ch, rb, cap, arity, engine=eng, final_poly_coeff_len=flen,
                                                     max_num_query_steps=steps)
    for t, d in zip(trees, o["digests"]):   # paths gathered on the device from the Keccak digest slots
        if len(d):
            want_path = kr.to_slots(np.array(kr.prove(d, 1, t.n_leaves, cap), dtype=np.uint8).reshape(-1, n_hash))
            assert (t.prove(1) == want_path).all()
    _check_commit(eng, trees, final, betas, ch, o, want, cap, n_hash)


# ---------------------------------------------------------------- 4. the grind
@pytest.mark.parametrize("pow_bits", [0, 1, 10])
@pytest.mark.parametrize("input_len", [0, 3, 7])
def test_grind_vs_reference(eng, pow_bits, input_len):
    from plonky2_amd.fri.prover import fri_proof_of_work
    rng = np.random.default_rng(17 * pow_bits + input_len)
    pre = rand_field(rng, 8 + input_len)
    ch, ref = _challenger(eng), kf.Challenger()
    ch.observe_elements(pre)
    ref.observe_elements(pre)
    assert len(ref.input_buffer) == input_len
    want = kf.fri_proof_of_work(ref, pow_bits)
    assert fri_proof_of_work(ch, pow_bits, engine=eng) == want
    _same(ch, ref)
    assert ch.get_n_challenges(2) == ref.get_n_challenges(2)


def test_grind_and_transcript_through_a_rejection_state(eng):
    from plonky2_amd.fri.prover import fri_proof_of_work
    c = REJECTION_STATES[0][0]
    state = [c] + [0] * 11
    # the candidate overwrites word 0 (input_len = 0): the candidate c itself is the rejection state
    ch, ref = _challenger(eng), _ref_at(state)
    _load(ch, state)
    assert kf.fri_proof_of_work(ref, 0) == 0 and fri_proof_of_work(ch, 0, engine=eng) == 0
    _same(ch, ref)
    # the same state through the transcript: observe c into an empty sponge, draw
    ch, ref = _challenger(eng), kf.Challenger()
    ch.observe_element(c)
    ref.observe_element(c)
    got = ch.get_challenge()
    assert got == ref.get_challenge() == REJECTION_STATES[0][4]   # the response is kept word 7
    _same(ch, ref)
    # ... and as the witness of a transcript: observed, the response drawn through the four-hash path
    ch, ref = _challenger(eng), kf.Challenger()
    for x in (ch, ref):
        x.observe_elements([REJECTION_STATES[1][0]])
    assert ch.get_n_challenges(8) == ref.get_n_challenges(8)
    _same(ch, ref)


# ---------------------------------------------------------------- 5. the whole opening proof
def _flip(words, byte=0):
    a = np.array(words, dtype=np.uint64, copy=True)
    a.reshape(-1).view(np.uint8)[byte] ^= 1
    return a


def test_whole_opening_proof(eng, ora):
    from plonky2_amd.fri.oracle import FriBatchInfo, PolynomialBatch, prove_openings
    from oracle import fri_verifier as fv
    from tests import pyref
    rng = np.random.default_rng(55)
    log_n, rb, cap, arity, Q, pow_bits, n_hash = 5, 3, 1, [2, 1], 3, 6, 25
    n, N = 1 << log_n, 1 << (log_n + rb)
    hasher, ref_h = _khash(eng, n_hash), kr.KeccakHash(n_hash)
    cols = [rand_field(rng, 3, n), rand_field(rng, 5, n)]
    salts = rand_field(rng, 4, N)
    oracles = [PolynomialBatch.from_coeffs(cols[0], rb, True, cap, engine=eng, salts=salts, hasher=hasher),
               PolynomialBatch.from_coeffs(cols[1], rb, False, cap, engine=eng, hasher=hasher)]
    leaves = [ora.commit_salted(cols[0], salts, rb, cap, False)["leaves"], ora.commit(cols[1], rb, cap, False)["leaves"]]
    all_polys = [(oi, pi) for oi, c in enumerate(cols) for pi in range(c.shape[0])]
    z0, z1 = rand_field(rng, 2), rand_field(rng, 2)
    ob = [(z0, all_polys), (z1, [(1, 0), (1, 3)])]
    batches = [FriBatchInfo(p, polys) for p, polys in ob]
    pre = rand_field(rng, 6)
    ch, ref = _challenger(eng, n_hash), kf.Challenger()
    ch.observe_elements(pre)
    ref.observe_elements(pre)
    verifier_transcript = ref.clone()
    want = kf.prove_openings(ob, cols, leaves, ref, rb, cap, arity, pow_bits, Q, ref_h)
    proof = prove_openings(batches, oracles, ch, rb, cap, arity, pow_bits, Q, engine=eng)
    # every buffer of the proof
    assert proof["pow_witness"] == want["pow_witness"] and proof["query_indices"] == want["query_indices"]
    assert (proof["final_poly"] == want["final_poly"]).all()
    for a, b in zip(proof["commit_phase_merkle_caps"], want["commit_phase_merkle_caps"]):
        assert (a == b).all()
    for qa, qb in zip(proof["query_round_proofs"], want["query_round_proofs"]):
        for (la, sa), (lb, sb) in zip(qa["initial_trees_proof"] + qa["steps"], qb["initial_trees_proof"] + qb["steps"]):
            assert (np.asarray(la) == lb).all() and (np.asarray(sa) == sb).all()
    for o, c in zip(oracles, want["initial_caps"]):
        assert (o.merkle_tree.cap.entries == kr.to_slots(c)).all()
    _same(ch, ref)
    # the Keccak verifier accepts it ...
    openings = [[pyref.ext_eval([(int(x) % P, 0) for x in cols[oi][pi]], (int(pt[0]), int(pt[1]))) for (oi, pi) in polys]
                for pt, polys in ob]

    def verify(pr):
        chal = kf.fri_challenges(verifier_transcript.clone(), pr, log_n, rb, cap, Q, ref_h)
        kf.verify_fri_proof(ob, openings, chal, want["initial_caps"], pr, log_n, rb, cap, arity, pow_bits, Q, ref_h)

    verify(proof)

    # ... and rejects a flipped byte in a cap, an initial path, a step path, final_poly, and another witness
    def tampered(**kw):
        p = dict(proof)
        p.update(kw)
        return p

    caps = [c.copy() for c in proof["commit_phase_merkle_caps"]]
    caps[0] = _flip(caps[0])
    q0 = proof["query_round_proofs"][0]
    init = list(q0["initial_trees_proof"])
    init[1] = (init[1][0], _flip(init[1][1]))
    steps = list(q0["steps"])
    steps[0] = (steps[0][0], _flip(steps[0][1]))
    rest = proof["query_round_proofs"][1:]
    for bad in (tampered(commit_phase_merkle_caps=caps),
                tampered(query_round_proofs=[{"initial_trees_proof": init, "steps": q0["steps"]}] + rest),
                tampered(query_round_proofs=[{"initial_trees_proof": q0["initial_trees_proof"], "steps": steps}] + rest),
                tampered(final_poly=_flip(proof["final_poly"])),
                tampered(pow_witness=proof["pow_witness"] + 1)):
        with pytest.raises(fv.VerificationError):
            verify(bad)


# ---------------------------------------------------------------- 6. boundaries
def test_boundaries(eng):
    from plonky2_amd.fri.oracle import FriBatchInfo, PolynomialBatch, prove_openings
    from plonky2_amd.iop.challenger import Challenger
    rng = np.random.default_rng(6)
    W, log_n, rb, cap = 4, 5, 2, 1
    vals = rand_field(rng, W, 1 << log_n)
    k25 = PolynomialBatch.from_values(vals, rb, False, cap, engine=eng, hasher=_khash(eng, 25))
    k32 = PolynomialBatch.from_values(vals, rb, False, cap, engine=eng, hasher=_khash(eng, 32))
    pb = PolynomialBatch.from_values(vals, rb, False, cap, engine=eng)
    kc, pc = _challenger(eng, 25), Challenger(eng)
    one = [FriBatchInfo([1, 2], [(0, 0)])]
    two = [FriBatchInfo([1, 2], [(0, 0), (1, 0)])]
    for batches, oracles, ch in ((one, [pb], kc), (two, [k25, k32], kc), (two, [k25, pb], kc), (one, [k25], pc), (one, [k32], kc)):
        before = ch.compact()
        with pytest.raises(_lib.P2HotError) as e:
            prove_openings(batches, oracles, ch, rb, cap, [1], 0, 2, engine=eng)
        assert e.value.code == _lib.EUNSUPPORTED and "Keccak" in str(e.value)
        assert ch.compact() == before
    # prove_openings_many stays Poseidon-only: a Keccak oracle, or a Keccak transcript
    ab = (C.c_uint * 1)(1)
    fp = _lib.FriParams(rb, cap, 0, 2, ab, 1, 0, 0, 0)
    oi, pi = (C.c_uint32 * 1)(0), (C.c_uint32 * 1)(0)
    info = (_lib.FriBatchInfo * 1)()
    info[0].point[0], info[0].point[1], info[0].oracle_index, info[0].poly_index, info[0].n_polys = 1, 2, oi, pi, 1
    infos = (C.POINTER(_lib.FriBatchInfo) * 1)(info)
    nb = (C.c_size_t * 1)(1)
    proofs = (_lib.FriProof * 1)()
    for batch, ch in ((k25, kc), (k25, pc), (pb, kc)):
        handles = (C.c_void_p * 1)(batch._h)
        chs = (C.c_void_p * 1)(ch._h)
        rc = eng.lib.p2hot_prove_openings_many(eng.ctx, 1, infos, nb, handles, 1, chs, C.byref(fp), proofs)
        assert rc == _lib.EUNSUPPORTED and "Keccak" in eng.lib.p2hot_last_error(eng.ctx).decode()
    # hash sizes
    for bad in (0, 33):
        h = C.c_void_p()
        assert eng.lib.p2hot_challenger_create_keccak(eng.ctx, bad, C.byref(h)) == _lib.EINVAL and not h
    # every handle is still usable: matching hashers prove, on both sides
    assert len(prove_openings(one, [k25], kc, rb, cap, [1], 0, 2, engine=eng)["query_round_proofs"]) == 2
    assert len(prove_openings(one, [pb], pc, rb, cap, [1], 0, 2, engine=eng)["query_round_proofs"]) == 2
    k32c = _challenger(eng, 32)
    assert len(prove_openings(one, [k32], k32c, rb, cap, [1], 0, 2, engine=eng)["query_round_proofs"]) == 2


# ---------------------------------------------------------------- 7. beyond one workgroup
@pytest.mark.gpu
def test_commit_phase_and_grind_beyond_one_workgroup(gpu, ora):
    """n = 2^14, rate 3, cap 4, arities [4, 4, 4], pow_bits 16 (the reference's witness search is about 2^16 numpy-vectorised
    permutations): round caps, betas, the final polynomial and the witness against the reference, digests by SHA-256"""
    from plonky2_amd.fri.prover import fri_committed_trees, fri_proof_of_work
    rng = np.random.default_rng(14)
    log_n, rb, cap, arity, pow_bits, n_hash = 14, 3, 4, [4, 4, 4], 16, 25
    coeffs = rand_field(rng, 1 << log_n, 2)
    ch, ref = _challenger(gpu, n_hash), kf.Challenger()
    trees, final, betas = fri_committed_trees(coeffs, ch, rb, cap, arity, engine=gpu)
    o = kf.fri_committed_trees(coeffs, ref, rb, cap, arity, kr.KeccakHash(n_hash))
    assert (np.asarray(betas) == o["betas"]).all() and (np.asarray(final) == o["final"]).all()
    for t, d, c in zip(trees, o["digests"], o["caps"]):
        assert (t.cap.entries == kr.to_slots(c)).all()
        got = np.ascontiguousarray(np.asarray(t.digests, dtype=np.uint64).reshape(-1, 4))
        assert hashlib.sha256(got.tobytes()).digest() == hashlib.sha256(np.ascontiguousarray(kr.to_slots(d)).tobytes()).digest()
    _same(ch, ref)
    assert fri_proof_of_work(ch, pow_bits, engine=gpu) == kf.fri_proof_of_work(ref, pow_bits, first_batch=1 << 14)
    _same(ch, ref)
