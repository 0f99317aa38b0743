"""The FRI opening proof of KeccakGoldilocksConfig restated from the Rust sources, on top of tests/keccak_ref.py (which the suite
pins to hashlib and the public Keccak-256 vectors).  TEST INFRASTRUCTURE ONLY; it never calls libp2hot.

  plonky2/src/hash/keccak.rs:63-94          KeccakPermutation::permute
  plonky2/src/iop/challenger.rs:30-153      Challenger (generic over the permutation)
  plonky2/src/hash/hash_types.rs:184-194    BytesHash<N>::to_vec
  plonky2/src/fri/prover.rs:84-150          fri_committed_trees (both padding options)
  plonky2/src/fri/prover.rs:153-202         fri_proof_of_work (smallest witness)
  plonky2/src/fri/prover.rs:204-258         fri_prover_query_rounds
  plonky2/src/fri/oracle.rs:176-237         PolynomialBatch::prove_openings
  plonky2/src/fri/challenges.rs:28-87, fri/verifier.rs:62-245   the verifier, with Keccak Merkle proofs

The hasher-independent arithmetic (transforms, reduce_polys_base, divide_by_linear, the verifier's interpolation) comes from the
CPU oracle and oracle/fri_verifier.py unchanged.
"""
import numpy as np

from oracle import fri_verifier as fv
from tests import keccak_ref as kr
from tests import ntt_ref

P = kr.P
RATE = 8
COSET_SHIFT = fv.MULTIPLICATIVE_GROUP_GENERATOR


# ------------------------------------------------------------------ KeccakPermutation (hash/keccak.rs:63-94)
def hash_stream(state, n_hashes):
    """the first 4 * n_hashes words of the hash onion of one state, before the rejection"""
    msg = kr.field_bytes(np.asarray(state, dtype=np.uint64).reshape(1, 12))
    out = []
    for _ in range(n_hashes):
        msg = kr.keccak256(msg)
        out += [int(w) for w in msg.view("<u8").reshape(-1)]
    return out


def permute(states):
    """[count][12] uint64 (any representatives) -> [count][12]: the first 12 words < p of each state's hash onion"""
    states = np.asarray(states, dtype=np.uint64).reshape(-1, 12)
    count = states.shape[0]
    msg = kr.field_bytes(states)
    out = np.zeros((count, 12), dtype=np.uint64)
    kept = np.zeros(count, dtype=np.int64)
    rows = np.arange(count)
    while (kept < 12).any():
        msg = kr.keccak256(msg)
        words = np.ascontiguousarray(msg).view("<u8").reshape(count, 4).astype(np.uint64)
        for i in range(4):
            keep = (words[:, i] < np.uint64(P)) & (kept < 12)   # rejection sampling: words that do not fit in F are ignored
            out[rows[keep], kept[keep]] = words[keep, i]
            kept += keep
    return out


def bytes_hash_to_vec(digest):
    """BytesHash<N>::to_vec: chunks of 7 bytes, each zero-extended to a u64"""
    d = bytes(np.asarray(digest, dtype=np.uint8))
    return [int.from_bytes(d[i:i + 7], "little") for i in range(0, len(d), 7)]


class Challenger:
    """Challenger<F, KeccakHash<N>>"""

    def __init__(self):
        self.sponge_state = [0] * 12
        self.input_buffer = []
        self.output_buffer = []

    def clone(self):
        c = Challenger()
        c.sponge_state, c.input_buffer, c.output_buffer = list(self.sponge_state), list(self.input_buffer), list(self.output_buffer)
        return c

    def observe_element(self, e):
        self.output_buffer = []
        self.input_buffer.append(int(e) % P)
        if len(self.input_buffer) == RATE:
            self.duplexing()

    def observe_elements(self, es):
        for e in np.asarray(es, dtype=np.uint64).reshape(-1):
            self.observe_element(e)

    def observe_hash(self, digest):
        self.observe_elements(bytes_hash_to_vec(digest))

    def observe_cap(self, cap):
        for d in cap:
            self.observe_hash(d)

    def get_challenge(self):
        if self.input_buffer or not self.output_buffer:
            self.duplexing()
        return self.output_buffer.pop()

    def get_n_challenges(self, n):
        return [self.get_challenge() for _ in range(n)]

    def get_extension_challenge(self):
        return self.get_n_challenges(2)

    def duplexing(self):
        assert len(self.input_buffer) <= RATE
        self.sponge_state[:len(self.input_buffer)] = self.input_buffer   # overwrite mode
        self.input_buffer = []
        self.sponge_state = [int(x) for x in permute(np.array(self.sponge_state, dtype=np.uint64))[0]]
        self.output_buffer = self.sponge_state[:RATE]

    def snapshot(self):
        """(sponge_state, input_buffer, output_buffer): what plonky2_amd's Challenger.compact() returns"""
        return (list(self.sponge_state), list(self.input_buffer), list(self.output_buffer))


# ------------------------------------------------------------------ F_p^2 on uint64 arrays
def _ext_mul(a0, a1, b0, b1):
    return (ntt_ref.add(ntt_ref.mul(a0, b0), ntt_ref.mul(np.uint64(7), ntt_ref.mul(a1, b1))),
            ntt_ref.add(ntt_ref.mul(a0, b1), ntt_ref.mul(a1, b0)))


def _fold(coeffs, arity, beta):
    """reduce_with_powers(chunk, beta) per chunk of `arity` coefficients (plonk_common.rs:120-132); coeffs [m][2]"""
    c = coeffs.reshape(-1, arity, 2)
    b0, b1 = np.uint64(beta[0]), np.uint64(beta[1])
    a0 = np.zeros(c.shape[0], dtype=np.uint64)
    a1 = np.zeros(c.shape[0], dtype=np.uint64)
    for i in reversed(range(arity)):
        a0, a1 = _ext_mul(a0, a1, b0, b1)
        a0, a1 = ntt_ref.add(a0, c[:, i, 0]), ntt_ref.add(a1, c[:, i, 1])
    return np.stack([a0, a1], axis=1)


def _coset_values(coeffs, rate_bits, shift):
    """coeffs.lde(rate_bits).coset_fft(shift) then reverse_index_bits, componentwise (the roots of unity are base-field)"""
    from oracle import p2oracle as ora
    n = coeffs.shape[0]
    planes = []
    for k in range(2):
        pad = np.zeros(n << rate_bits, dtype=np.uint64)
        pad[:n] = coeffs[:, k]
        planes.append(ora.reverse_index_bits(ora.coset_fft(pad, shift)))
    return np.stack(planes, axis=1)


# ------------------------------------------------------------------ fri_committed_trees (fri/prover.rs:84-150)
def fri_committed_trees(coeffs, challenger, rate_bits, cap_height, arity_bits, hasher, final_poly_coeff_len=None,
                        max_num_query_steps=None):
    """coeffs [n][2]: the nonzero coefficients.  Returns dict(leaves, digests, caps: per round, digests as uint8 [..][N]; betas, final)"""
    coeffs = ntt_ref.reduce(np.asarray(coeffs, dtype=np.uint64))
    out = dict(leaves=[], digests=[], caps=[], betas=[], final=None)
    shift = COSET_SHIFT
    for ab in arity_bits:
        arity = 1 << ab
        values = _coset_values(coeffs, rate_bits, shift)
        leaves = values.reshape(-1, 2 * arity)                 # par_chunks(arity) + flatten
        digests, cap = kr.merkle_tree(leaves, cap_height, hasher)
        challenger.observe_cap(cap)
        beta = challenger.get_extension_challenge()
        out["leaves"].append(leaves)
        out["digests"].append(digests)
        out["caps"].append(cap)
        out["betas"].append(beta)
        coeffs = _fold(coeffs, arity, beta)
        shift = pow(shift, arity, P)
    if max_num_query_steps is not None:
        zero_cap = np.zeros((1 << cap_height) * 4, dtype=np.uint64)   # NUM_HASH_OUT_ELTS = 4, whatever the hasher
        for _ in range(len(arity_bits), max_num_query_steps):
            challenger.observe_elements(zero_cap)
            challenger.get_extension_challenge()
    challenger.observe_elements(coeffs.reshape(-1))
    if final_poly_coeff_len is not None:
        for _ in range(coeffs.shape[0], final_poly_coeff_len):
            challenger.observe_elements([0, 0])
    out["final"] = coeffs
    out["betas"] = np.array(out["betas"], dtype=np.uint64).reshape(-1, 2)
    return out


# ------------------------------------------------------------------ fri_proof_of_work (fri/prover.rs:153-202)
def fri_proof_of_work(challenger, pow_bits, first_batch=1024):
    """the SMALLEST witness, then observe it and draw the response like the reference"""
    inter = list(challenger.sponge_state)
    pos = len(challenger.input_buffer)
    inter[:pos] = challenger.input_buffer
    start, batch, witness = 0, first_batch, None
    while witness is None:
        cand = np.arange(start, start + batch, dtype=np.uint64)
        st = np.tile(np.array(inter, dtype=np.uint64), (batch, 1))
        st[:, pos] = cand
        resp = permute(st)[:, RATE - 1]
        ok = np.nonzero(resp >> np.uint64(64 - pow_bits) == 0)[0] if pow_bits else np.arange(batch)
        if ok.size:
            witness = int(cand[ok[0]])
        start += batch
        batch = min(2 * batch, 1 << 16)
    challenger.observe_element(witness)
    response = challenger.get_challenge()
    assert 64 - response.bit_length() >= pow_bits
    return witness


# ------------------------------------------------------------------ prove_openings (fri/oracle.rs:176-237) + fri_proof
def final_poly(batches, coeff_sets, alpha):
    """sum_i alpha^(k_i) (F_i - F_i(z_i)) / (X - z_i); batches: [(point, [(oracle, poly), ...])] -> [n][2]"""
    from oracle import p2oracle as ora
    n = coeff_sets[0].shape[1]
    a = (int(alpha[0]), int(alpha[1]))
    final = np.zeros((n, 2), dtype=np.uint64)
    for point, polys in batches:
        ps = np.stack([coeff_sets[o][p] for (o, p) in polys])
        quo = ora.divide_by_linear(ora.reduce_polys_base(ps, np.array(alpha, dtype=np.uint64)), np.asarray(point, dtype=np.uint64))
        sh = fv.e_pow(a, len(polys))                           # shift_poly
        f0, f1 = _ext_mul(final[:, 0], final[:, 1], np.uint64(sh[0]), np.uint64(sh[1]))
        final = np.stack([ntt_ref.add(f0, quo[:, 0]), ntt_ref.add(f1, quo[:, 1])], axis=1)
    return final


def prove_openings(batches, coeff_sets, initial_leaves, challenger, rate_bits, cap_height, arity_bits, pow_bits, num_queries,
                   hasher, final_poly_coeff_len=None, max_num_query_steps=None):
    """initial_leaves: per oracle the [N][leaf width] leaf matrix (salts included).  Returns the FriProof-shaped dict of
    plonky2_amd.fri.oracle.prove_openings, digests as 32-byte slots, plus "initial_caps" (uint8) for the verifier."""
    n = coeff_sets[0].shape[1]
    N = n << rate_bits
    alpha = challenger.get_extension_challenge()
    fin = final_poly(batches, coeff_sets, alpha)
    o = fri_committed_trees(fin, challenger, rate_bits, cap_height, arity_bits, hasher, final_poly_coeff_len, max_num_query_steps)
    witness = fri_proof_of_work(challenger, pow_bits)
    initial = [kr.merkle_tree(lv, cap_height, hasher) for lv in initial_leaves]
    queries, indices = [], []
    for rand in challenger.get_n_challenges(num_queries):
        x = rand % N
        indices.append(x)
        init = [(lv[x], kr.to_slots(np.array(kr.prove(d, x, N, cap_height), dtype=np.uint8).reshape(-1, hasher.n)))
                for lv, (d, _) in zip(initial_leaves, initial)]
        steps = []
        for i, ab in enumerate(arity_bits):
            lv, d = o["leaves"][i], o["digests"][i]
            sib = np.array(kr.prove(d, x >> ab, lv.shape[0], cap_height), dtype=np.uint8).reshape(-1, hasher.n)
            steps.append((lv[x >> ab].reshape(-1, 2), kr.to_slots(sib)))
            x >>= ab
        queries.append({"initial_trees_proof": init, "steps": steps})
    return {"commit_phase_merkle_caps": [kr.to_slots(c) for c in o["caps"]], "query_round_proofs": queries, "final_poly": o["final"],
            "pow_witness": witness, "query_indices": indices, "initial_caps": [c for _, c in initial]}


# ------------------------------------------------------------------ the verifier
def fri_challenges(challenger, proof, degree_bits, rate_bits, cap_height, num_queries, hasher, final_poly_coeff_len=None,
                   max_num_query_steps=None):
    """fri/challenges.rs:28-87 with observe_cap of BytesHash<N> caps"""
    lde_size = 1 << (degree_bits + rate_bits)
    alpha = fv.e_of(challenger.get_extension_challenge())
    betas = []
    for cap in proof["commit_phase_merkle_caps"]:
        challenger.observe_cap(kr.from_slots(cap, hasher.n))
        betas.append(fv.e_of(challenger.get_extension_challenge()))
    if max_num_query_steps is not None:
        for _ in range(len(betas), max_num_query_steps):
            challenger.observe_elements(np.zeros((1 << cap_height) * 4, dtype=np.uint64))
            challenger.get_extension_challenge()
    fp = np.asarray(proof["final_poly"], dtype=np.uint64).reshape(-1)
    challenger.observe_elements(fp)
    if final_poly_coeff_len is not None:
        for _ in range(fp.size // 2, final_poly_coeff_len):
            challenger.observe_elements([0, 0])
    challenger.observe_element(proof["pow_witness"])
    response = challenger.get_challenge()
    return {"fri_alpha": alpha, "fri_betas": betas, "fri_pow_response": response,
            "fri_query_indices": [challenger.get_challenge() % lde_size for _ in range(num_queries)]}


def _verify_merkle(leaf, index, cap, siblings, cap_height, hasher):
    leaf = np.asarray(leaf, dtype=np.uint64).reshape(1, -1)
    path = kr.from_slots(siblings, hasher.n) if len(siblings) else []
    if not kr.verify(hasher.hash_or_noop(leaf)[0], int(index), path, cap, cap_height, hasher):
        raise fv.VerificationError("Invalid Merkle proof.")


def verify_fri_proof(batches, openings, challenges, initial_caps, proof, degree_bits, rate_bits, cap_height, arity_bits, pow_bits,
                     num_queries, hasher):
    """verify_fri_proof / fri_verifier_query_round (fri/verifier.rs:62-245) over Keccak trees.  batches: [(point, [(oracle,
    poly)...])]; openings: per batch the opened values [[c0, c1]...]; initial_caps: uint8 [2^cap_height][N] per oracle"""
    n = 1 << (degree_bits + rate_bits)
    if len(proof["commit_phase_merkle_caps"]) != len(arity_bits):
        raise fv.VerificationError("shape: commit phase caps")
    if len(np.asarray(proof["final_poly"]).reshape(-1, 2)) != (1 << degree_bits) >> sum(arity_bits):
        raise fv.VerificationError("shape: final polynomial length")
    fv.fri_verify_proof_of_work(challenges["fri_pow_response"], pow_bits)
    if num_queries != len(proof["query_round_proofs"]):
        raise fv.VerificationError("Number of query rounds does not match config.")
    reduced = [fv.ReducingFactor(challenges["fri_alpha"]).reduce([fv.e_of(v) for v in vals]) for vals in openings]
    caps = [kr.from_slots(c, hasher.n) for c in proof["commit_phase_merkle_caps"]]
    log_n = degree_bits + rate_bits
    for x_index, rp in zip(challenges["fri_query_indices"], proof["query_round_proofs"]):
        init = rp["initial_trees_proof"]
        if len(init) != len(initial_caps):
            raise fv.VerificationError("shape: initial trees")
        for (evals, path), cap in zip(init, initial_caps):                                   # fri_verify_initial_proof
            _verify_merkle(evals, x_index, cap, path, cap_height, hasher)
        subgroup_x = COSET_SHIFT * pow(fv.ora.root_of_unity(log_n), fv.reverse_bits(x_index, log_n), P) % P
        old_eval = fv.fri_combine_initial(batches, init, challenges["fri_alpha"], subgroup_x, reduced)
        for i, ab in enumerate(arity_bits):
            arity = 1 << ab
            flat = np.asarray(rp["steps"][i][0], dtype=np.uint64)
            evals = [fv.e_of(v) for v in flat.reshape(-1, 2)]
            if len(evals) != arity:
                raise fv.VerificationError("shape: step evals")
            coset_index, within = x_index >> ab, x_index & (arity - 1)
            if evals[within] != old_eval:
                raise fv.VerificationError("FRI step %d is inconsistent with the previous evaluation" % i)
            old_eval = fv.compute_evaluation(subgroup_x, within, ab, evals, challenges["fri_betas"][i])
            _verify_merkle(flat.reshape(-1), coset_index, caps[i], rp["steps"][i][1], cap_height, hasher)
            subgroup_x = pow(subgroup_x, arity, P)
            x_index = coset_index
        acc, sx = (0, 0), fv.e_from_base(subgroup_x)
        for c in reversed([fv.e_of(c) for c in np.asarray(proof["final_poly"], dtype=np.uint64).reshape(-1, 2)]):
            acc = fv.e_add(fv.e_mul(acc, sx), c)
        if acc != old_eval:
            raise fv.VerificationError("Final polynomial evaluation is invalid.")
