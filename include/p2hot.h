/*
 * p2hot.h -- C ABI of libp2hot: the MI355X (gfx950) implementation of plonky2's
 * PolynomialBatch LDE + Poseidon-Merkle commit pipeline and FRI commit phase.
 *
 * This is the drop-in boundary a patched `plonky2` crate binds with `extern "C"` (see
 * INTEGRATION.md).  The reference has no plugin trait for this path; each entry point cites the
 * reference function whose body it replaces (paths relative to the plonky2 repository).
 *
 * Conventions
 *  - Field elements are uint64_t (GoldilocksField is #[repr(transparent)] u64,
 *    field/src/goldilocks_field.rs:23-25).  Inputs may be any representative < 2^64; every value
 *    written to an output buffer is canonical (< P = 2^64 - 2^32 + 1).
 *  - Extension elements (F^2) are two consecutive words [a0, a1] (field/src/extension/quadratic.rs:13).
 *  - Digests are 4 words (hash/hash_types.rs:25-27).
 *  - Functions return 0 (P2HOT_OK) or a P2HOT_E* code; p2hot_last_error() has the text.  No C++
 *    exception, abort or library-owned host memory crosses this boundary.
 *  - `*_dev` functions take DEVICE pointers and only enqueue work on the context's HIP stream;
 *    the others take HOST pointers, stage through device memory owned by the context and return
 *    after the results are in the caller's buffers.
 *  - A context is bound to one GPU and runs one call at a time; use one context per GPU (one process per GPU with
 *    p2hot_comm_*, or one process for all GPUs with p2hot_group_*, see the multi-GPU section).
 */
#ifndef P2HOT_H
#define P2HOT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P2HOT_OK 0
#define P2HOT_EINVAL 1       /* bad shape / argument (the reference would panic!, e.g. fft.rs:171, merkle_tree.rs:195) */
#define P2HOT_ENOMEM 2       /* device allocation failed */
#define P2HOT_EHIP 3         /* HIP runtime error */
#define P2HOT_EUNSUPPORTED 4 /* valid in the reference but not on this path */

#define P2HOT_P 0xFFFFFFFF00000001ULL
#define P2HOT_COSET_SHIFT 14293326489335486720ULL /* F::coset_shift(), field/src/goldilocks_field.rs:80 */

typedef struct p2hot_ctx p2hot_ctx;

/* ---------------------------------------------------------------- context */
/* hip_stream: the hipStream_t all work of this context is enqueued on; NULL = the legacy default
 * stream (which is also PyTorch's default stream).  The caller keeps the stream alive. */
int p2hot_ctx_create(int device, void *hip_stream, p2hot_ctx **out);
void p2hot_ctx_destroy(p2hot_ctx *ctx);
int p2hot_ctx_set_stream(p2hot_ctx *ctx, void *hip_stream);
int p2hot_ctx_sync(p2hot_ctx *ctx);
const char *p2hot_last_error(const p2hot_ctx *ctx);
const char *p2hot_version(void);
/* 1 when the library was built by the test-only kernel emulator (tests/emu), 0 for the HIP build */
int p2hot_is_emulated(void);

/* Live per-kernel timing: when enabled, the launches of each kernel family are bracketed with HIP
 * events on the context's stream.  p2hot_profile_json synchronises, drains them and returns
 * {"kernel": {"ms": total, "launches": count}, ...} (valid until the next call); reset != 0 clears
 * the totals.  This is the TimingTree analogue (plonky2/src/util/timing.rs) for the GPU stages. */
int p2hot_profile_enable(p2hot_ctx *ctx, int on);
/* tuning knob for the NTT pass kernels (0 = LDS radix-2 layers, 3 = register radix 8 on carry-free 24-bit limbs
 * [default; 4096-element tiles, other tiles as 8], 8 = register radix 8 on 64-bit words, 4 = radix 16);
 * results are identical, only the speed differs.  ABI note: until round 2 `3` meant the 64-bit-word radix-8 kernels, which are
 * `8` now; P2HOT_NTT_LIMB=0 in the environment is sticky (then `3` selects the word kernels as before). */
int p2hot_tune_ntt(p2hot_ctx *ctx, int radix_bits);
/* overlap the Poseidon leaf sponge of coset block b with the LDE of block b+1 on a second HIP stream (default 0: measured neutral on MI355X) */
int p2hot_tune_overlap(p2hot_ctx *ctx, int on);
/* leaf-hash / tree-level launches with at most max_perms permutations run the quad-cooperative kernels (4 lanes per
 * permutation, ~3x lower latency, 1.3x the work); default 2^15, 0 = never.  Results are identical. */
int p2hot_tune_quad(p2hot_ctx *ctx, size_t max_perms);
/* ... and launches with at most max_perms permutations the word-per-lane kernels (16 lanes per permutation, one state word
 * and one MDS row per lane through DPP row broadcasts: ~3x lower latency than the quad kernels, ~3.6x the work); default 2^13, 0 = never.
 * The Fiat-Shamir sponge always runs this mapping.  Results are identical. */
int p2hot_tune_row(p2hot_ctx *ctx, size_t max_perms);
const char *p2hot_profile_json(p2hot_ctx *ctx, int reset);

/* sizes: number of digests (4 words each) in MerkleTree::digests for n_leaves = 2^log_leaves
 * (hash/merkle_tree.rs:203: 2 * (n_leaves - 2^cap_height)) */
size_t p2hot_num_digests(unsigned log_leaves, unsigned cap_height);

/* ---------------------------------------------------------------- primitives (device pointers) */
/* fft_with_options(input, None, None) for `batch` polynomials, in place, natural order in and out:
 * out[i] = sum_t in[t] * w_n^(i*t)  (field/src/fft.rs:53-65).  poly_stride >= n elements. */
int p2hot_fft_dev(p2hot_ctx *ctx, uint64_t *d_data, size_t batch, size_t poly_stride, unsigned log_n);
/* ifft_with_options (field/src/fft.rs:68-91): values on H_n -> coefficients, in place. */
int p2hot_ifft_dev(p2hot_ctx *ctx, uint64_t *d_data, size_t batch, size_t poly_stride, unsigned log_n);
/* PolynomialValues::coset_ifft (field/src/polynomial/mod.rs:63-73): values on shift * H_n -> coefficients, in place
 * (the quotient-side transform of plonk/prover.rs:810-814) */
int p2hot_coset_ifft_dev(p2hot_ctx *ctx, uint64_t *d_data, size_t batch, size_t poly_stride, unsigned log_n,
                         uint64_t shift);
/* PolynomialBatch::lde_values (fri/oracle.rs:114-139) = lde(rate_bits) + coset_fft(shift) for W
 * polynomials, fused with the transpose + reverse_index_bits of oracle.rs:97-98:
 *   d_lde[c * lde_stride + (L - row_begin)] = p_c(shift * w_N^bitrev(L)),  L in [row_begin, row_begin + row_count)
 * where N = n << rate_bits.  Rows are produced in whole coset blocks of n rows: row_begin and
 * row_count must be multiples of n (row block b holds coset j = bitrev_rb(b)). */
int p2hot_coset_lde_dev(p2hot_ctx *ctx, const uint64_t *d_coeffs, size_t W, size_t coeff_stride, unsigned log_n,
                        unsigned rate_bits, uint64_t shift, size_t row_begin, size_t row_count, uint64_t *d_lde,
                        size_t lde_stride);
/* transpose (plonky2/src/util/mod.rs:25-31): column-major [W][rows] -> row-major [rows][W], canonical */
int p2hot_transpose_dev(p2hot_ctx *ctx, const uint64_t *d_colmajor, size_t col_stride, size_t W, size_t rows,
                        uint64_t *d_rowmajor);
/* reverse_index_bits (util/src/lib.rs:53-62) on `batch` arrays of 2^log_n words, out of place */
int p2hot_reverse_index_bits_dev(p2hot_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, size_t batch,
                                 size_t poly_stride, unsigned log_n);
/* Poseidon::poseidon on `count` states of 12 words, in place (hash/poseidon.rs:767-777) */
int p2hot_poseidon_permute_dev(p2hot_ctx *ctx, uint64_t *d_states, size_t count);
/* MerkleTree::new (hash/merkle_tree.rs:193-224) for the leaf range [leaf_begin, leaf_begin + leaf_count)
 * of a tree with 2^log_leaves leaves; the range must be a whole number of cap subtrees.
 * layout: 0 = leaves column-major (element (L, c) at d_leaves[c * leaf_stride + L - leaf_begin]),
 *         1 = leaves row-major    (d_leaves[(L - leaf_begin) * W + c]).
 * d_digests / d_cap point at the FULL tree's arrays (reference layout, merkle_tree.rs:50-57);
 * only the entries of the given range are written. */
int p2hot_merkle_dev(p2hot_ctx *ctx, const uint64_t *d_leaves, int layout, size_t leaf_stride, size_t W,
                     unsigned log_leaves, unsigned cap_height, size_t leaf_begin, size_t leaf_count,
                     uint64_t *d_digests, uint64_t *d_cap);
/* ---------------------------------------------------------------- KeccakHash<N> (hash/keccak.rs:104-127)
 * Keccak-256 trees for KeccakGoldilocksConfig (plonk/config.rs:118-126).  A KeccakHash<N> digest (N = hash_size, 1..32 bytes;
 * 0 or > 32 is P2HOT_EINVAL) occupies bytes 0..N of the same 4-word slot a Poseidon digest does, bytes N..32 zero, so the
 * digest / cap arrays, p2hot_merkle_paths_dev and p2hot_batch_paths / _digests carry Keccak trees unchanged.
 * p2hot_keccak256_dev: `count` messages of msg_bytes bytes, back to back in d_msgs; d_out [count][4] the 32-byte output of the
 * sponge with rate 136 and the given domain byte (0x01 = Keccak-256 as keccak_hash::keccak, 0x06 = SHA3-256). */
int p2hot_keccak256_dev(p2hot_ctx *ctx, const uint8_t *d_msgs, size_t msg_bytes, size_t count, unsigned domain_byte,
                        uint64_t *d_out);
/* p2hot_merkle_dev for KeccakHash<hash_size>: MerkleTree::new with hash_or_noop on the leaves (plonk/config.rs:63-74: a leaf
 * of 8 * W <= hash_size bytes is its canonical bytes, zero-padded) and two_to_one = Keccak-256(left[0..N] || right[0..N]) */
int p2hot_keccak_merkle_dev(p2hot_ctx *ctx, const uint64_t *d_leaves, int layout, size_t leaf_stride, size_t W,
                            unsigned log_leaves, unsigned cap_height, size_t leaf_begin, size_t leaf_count,
                            uint64_t *d_digests, uint64_t *d_cap, unsigned hash_size);
/* Field-arithmetic self test (goldilocks_field.rs:245-320, :402-415): for count operand pairs writes six arrays of
 * `count` words to d_out: a*b by the compiler-scheduled multiply, by the hand-scheduled single stream, by the 3-way
 * interleaved stream, a+b, a-b (all canonical), and a word that is 0 unless a hand-written instruction stream disagreed
 * with the compiler-scheduled arithmetic (bit 0 the other two mul3 lanes, 1 the low-register multiply, 2 the
 * power-of-two twiddle multiplies, 3 / 4 the MDS row recombinations fold1 / fold3, 5 the two-stream mul2; 6 is reserved and never set). */
int p2hot_field_selftest_dev(p2hot_ctx *ctx, const uint64_t *d_a, const uint64_t *d_b, size_t count, uint64_t *d_out);
/* rows of a column-major matrix of `rows` rows: d_out[q][c] = d_colmajor[c * col_stride + d_idx[q]]
 * (PolynomialBatch::get_lde_values / MerkleTree::get, fri/oracle.rs:142-147, merkle_tree.rs:227).
 * The indices are device-resident, so they cannot be validated before the launch: an index >= rows reads nothing,
 * its output row is zero, and the next p2hot_ctx_sync returns P2HOT_EINVAL (the reference panics on the slice index). */
int p2hot_gather_rows_dev(p2hot_ctx *ctx, const uint64_t *d_colmajor, size_t col_stride, size_t rows, size_t W,
                          const uint64_t *d_idx, size_t m, uint64_t *d_out);

/* ---------------------------------------------------------------- PolynomialBatch (device pointers) */
/* PolynomialBatch::from_values (is_values != 0, fri/oracle.rs:57-79) / from_coeffs (:82-112) with
 * blinding = false, restricted to the leaf rows [row_begin, row_begin + row_count) (whole coset
 * blocks and whole cap subtrees; pass 0, N for the full commitment).
 *   d_cols    [W][n] column-major input (values on H_n, or coefficients), stride col_stride
 *   d_coeffs  [W][n] out: the coefficient form (`polynomials`); may alias d_cols when
 *             is_values == 0; NULL only when is_values == 0
 *   d_lde     [W][row_count] out: column-major LDE, rows in committed (bit-reversed) order,
 *             stride lde_stride -- the device-resident form of MerkleTree::leaves
 *   d_leaves  [row_count][W] out, row-major copy (the reference's `leaves`), or NULL
 *   d_digests, d_cap: FULL-tree arrays (see p2hot_merkle_dev) */
int p2hot_commit_dev(p2hot_ctx *ctx, const uint64_t *d_cols, size_t col_stride, size_t W, unsigned log_n,
                     unsigned rate_bits, unsigned cap_height, int is_values, size_t row_begin, size_t row_count,
                     uint64_t *d_coeffs, size_t coeff_stride, uint64_t *d_lde, size_t lde_stride,
                     uint64_t *d_leaves, uint64_t *d_digests, uint64_t *d_cap);

/* p2hot_commit_dev with the tree built by KeccakHash<hash_size> (the LDE does not depend on the hasher) */
int p2hot_commit_keccak_dev(p2hot_ctx *ctx, const uint64_t *d_cols, size_t col_stride, size_t W, unsigned log_n,
                            unsigned rate_bits, unsigned cap_height, int is_values, size_t row_begin, size_t row_count,
                            uint64_t *d_coeffs, size_t coeff_stride, uint64_t *d_lde, size_t lde_stride,
                            uint64_t *d_leaves, uint64_t *d_digests, uint64_t *d_cap, unsigned hash_size);

/* ---------------------------------------------------------------- Challenger (device-resident) */
/* plonky2/src/iop/challenger.rs:16-153.  The sponge lives on the GPU so FRI rounds need no host
 * round trip; the host (or the Rust shim) moves its state in and out with load/store. */
typedef struct {
    uint64_t sponge_state[12];
    uint64_t input_buffer[8];
    uint64_t output_buffer[8];
    uint32_t input_len, output_len;
} p2hot_challenger_state;
typedef struct p2hot_challenger p2hot_challenger;
int p2hot_challenger_create(p2hot_ctx *ctx, p2hot_challenger **out); /* Challenger::<F, PoseidonHash>::new */
/* Challenger::<F, KeccakHash<hash_size>>::new (KeccakGoldilocksConfig: hash_size = 25): the same handle, state layout and
 * load / store / step / destroy; the duplex (challenger.rs:129-144) runs KeccakPermutation (hash/keccak.rs:63-94: the state's 96
 * canonical bytes through a chain of Keccak-256 hashes, every output word >= p dropped).  hash_size is 1..32, else P2HOT_EINVAL.
 * The Keccak duplex is a chain of three dependent Keccak-f and runs on one lane: about 37 us per duplex, i.e. per 8 observed
 * elements (the Poseidon one: 10 us), so observing a long vector -- the final polynomial of a schedule with few reduction rounds,
 * a large final_poly_coeff_len -- costs that much per 8 elements on a single GPU thread.
 * The handle records its hasher: it is what selects the Keccak FRI trees and grind in p2hot_fri_commit / _dev, p2hot_fri_pow and
 * p2hot_prove_openings. */
int p2hot_challenger_create_keccak(p2hot_ctx *ctx, unsigned hash_size, p2hot_challenger **out);
void p2hot_challenger_destroy(p2hot_challenger *ch);
int p2hot_challenger_load(p2hot_challenger *ch, const p2hot_challenger_state *host_state);
int p2hot_challenger_store(p2hot_challenger *ch, p2hot_challenger_state *host_state);
/* observe_elements (challenger.rs:50-54) then get_n_challenges (:93-95); host pointers; either count may be 0 */
int p2hot_challenger_step(p2hot_challenger *ch, const uint64_t *observe, size_t n_observe, uint64_t *challenges,
                          size_t n_challenges);
/* observe_hash / observe_cap (challenger.rs:69-80) of `count` digests given as their 32-byte slots (host [count][4]): the
 * elements of GenericHashOut::to_vec.  A Poseidon challenger observes the 4 words of each; a KeccakHash<N> challenger the
 * ceil(N / 7) seven-byte chunks of bytes 0..N, each zero-extended to a word (hash_types.rs:184-194: 4 elements for N = 25, 5 for
 * N = 32); bytes N..32 of a slot are ignored. */
int p2hot_challenger_observe_digests(p2hot_challenger *ch, const uint64_t *slots, size_t count);

/* ---------------------------------------------------------------- FRI commit phase */
/* fri_committed_trees (fri/prover.rs:84-150) including the `lde_final_values` coset FFT of
 * prove_openings (fri/oracle.rs:215-220).  Host pointers.
 *   coeffs        [n][2]: the n = 2^log_n nonzero extension coefficients of final_poly (the
 *                 reference passes them zero-padded to N = n << rate_bits; the padding is implicit here)
 *   arity_bits    reduction_arity_bits (fri/reduction_strategies.rs:31-59), n_rounds entries
 *   challenger    advanced exactly like the reference: per round observe_cap then
 *                 get_extension_challenge; finally observe the final coefficients
 *   outputs (any may be NULL), concatenated over rounds r with m_r = N >> sum(arity_bits[0..r)):
 *     leaves_out   m_r * 2 words per round: tree r's leaves (m_r/arity rows of 2*arity words)
 *     digests_out  4 * p2hot_num_digests(log m_r - arity_bits[r], cap_height) words per round
 *     caps_out     4 << cap_height words per round
 *     betas_out    2 words per round
 *     final_out    [(m_last >> rate_bits)][2], m_last = N >> sum(arity_bits)
 * The round trees are built by the challenger's hasher: with a Keccak challenger (p2hot_challenger_create_keccak) they are
 * KeccakHash<N> trees (digests and caps in 32-byte slots, bytes N..32 zero; hash_or_noop copies a leaf of 8 * W <= N bytes, which
 * happens for N = 32 at arity 2), each cap is observed as BytesHash<N> digests, and the dummy caps of max_num_query_steps are 4 zero
 * elements per entry whatever the hasher (fri/prover.rs:126). */
int p2hot_fri_commit(p2hot_ctx *ctx, const uint64_t *coeffs, unsigned log_n, unsigned rate_bits,
                     unsigned cap_height, const unsigned *arity_bits, unsigned n_rounds,
                     unsigned max_num_query_steps, size_t final_poly_coeff_len,
                     p2hot_challenger *challenger, uint64_t *leaves_out, uint64_t *digests_out,
                     uint64_t *caps_out, uint64_t *betas_out, uint64_t *final_out);
/* max_num_query_steps / final_poly_coeff_len: the two Option<usize> arguments of fri_committed_trees
 * (fri/prover.rs:89-90, used by starky's multi-degree recursion: dummy cap observations + challenges up to
 * max_num_query_steps, :122-132, zero observations up to final_poly_coeff_len, :140-147); 0 = None. */
/* the same with the coefficients already on the device as two planes [2][n] (component 0, then component 1),
 * e.g. the output of p2hot_fri_final_poly_dev.  d_leaves_out is a DEVICE buffer (or NULL): the round trees' leaf
 * matrices stay on the GPU (same concatenated layout) and the query phase gathers the few rows it opens.
 * digests_out is a DEVICE buffer when digests_on_device != 0 (the round trees' digest arrays stay on the GPU next
 * to their leaves; Merkle paths then come from p2hot_merkle_paths_dev), else a host buffer; the other outputs are
 * host pointers as above. */
int p2hot_fri_commit_dev(p2hot_ctx *ctx, const uint64_t *d_coeffs_planar, unsigned log_n, unsigned rate_bits,
                         unsigned cap_height, const unsigned *arity_bits, unsigned n_rounds,
                         unsigned max_num_query_steps, size_t final_poly_coeff_len,
                         p2hot_challenger *challenger, uint64_t *d_leaves_out, uint64_t *digests_out,
                         int digests_on_device, uint64_t *caps_out, uint64_t *betas_out, uint64_t *final_out);
/* The final_poly construction of PolynomialBatch::prove_openings (fri/oracle.rs:186-213) on device-resident
 * coefficient polynomials: for every batch i with opening point z_i,
 *   F_i = ReducingFactor::reduce_polys_base(polys of the batch)      (util/reducing.rs:83-95)
 *   q_i = F_i.divide_by_linear(z_i), padded with a zero                 (field/src/polynomial/division.rs:79-92)
 *   final_poly = final_poly * alpha^(#polys of batch i) + q_i          (shift_poly, reducing.rs:103-106)
 * d_poly_table: DEVICE array of device pointers, each to n = 2^log_n base-field coefficients; batch i uses
 * entries [batch_offsets[i], batch_offsets[i+1]).  points [n_batches][2], alpha [2]: host.  d_final: planes [2][n]. */
int p2hot_fri_final_poly_dev(p2hot_ctx *ctx, const uint64_t *const *d_poly_table, const size_t *batch_offsets,
                             size_t n_batches, const uint64_t *points, const uint64_t alpha[2], unsigned log_n,
                             uint64_t *d_final);
/* OpeningSet::new (plonky2/src/plonk/proof.rs:314-327): evaluate n_polys device-resident coefficient
 * polynomials (d_poly_table: DEVICE array of device pointers, 2^log_n words each) at n_points extension points
 * (host [n_points][2]): d_out[p][j] = polys[j](points[p]) as [2] words, layout [n_points][n_polys][2]. */
int p2hot_eval_polys_dev(p2hot_ctx *ctx, const uint64_t *const *d_poly_table, size_t n_polys, unsigned log_n,
                         const uint64_t *points, size_t n_points, uint64_t *d_out);
/* all_wires_permutation_partial_products (plonky2/src/plonk/prover.rs:356-449): the permutation
 * argument's Z and partial-product polynomials (values on the trace subgroup) for num_challenges (beta, gamma) pairs.
 *   d_wires   DEVICE [num_routed][n] column-major (MatrixWitness.wire_values[col][row], iop/witness.rs:283-291)
 *   d_sigmas  DEVICE [num_routed][n] column-major: sigma_j(w_n^i) (the sigma polynomials' values; prover_data.sigmas
 *             holds their transpose)
 *   k_is      HOST [num_routed] coset shifts (common_data.k_is), betas / gammas HOST [num_challenges]
 *   degree    = common_data.quotient_degree_factor (chunk size); num_prods = ceil(num_routed / degree) - 1
 *   d_out     DEVICE [num_challenges * (num_prods + 1)][n], ordered as the prover batches them for the commit
 *             (prover.rs:224-229): Z of challenge 0 .. nc-1, then the num_prods partial products of challenge 0, 1, ...
 * Canonical outputs; feed d_out to p2hot_commit_dev(is_values = 1).  A zero denominator (the reference panics,
 * "Tried to invert zero") returns P2HOT_EINVAL. */
int p2hot_partial_products_dev(p2hot_ctx *ctx, const uint64_t *d_wires, size_t wires_stride, const uint64_t *d_sigmas,
                               size_t sigmas_stride, const uint64_t *k_is, unsigned num_routed, unsigned log_n,
                               unsigned degree, const uint64_t *betas, const uint64_t *gammas, unsigned num_challenges,
                               uint64_t *d_out, size_t out_stride);
/* merkle_tree_prove (hash/merkle_tree.rs:151-190) for m leaf indices from a device-resident digest array
 * (the query phase, fri/prover.rs:204-258): d_out [m][log_leaves - cap_height][4].  A leaf index
 * >= 2^log_leaves yields a zero path and P2HOT_EINVAL at the next p2hot_ctx_sync (see p2hot_gather_rows_dev). */
int p2hot_merkle_paths_dev(p2hot_ctx *ctx, const uint64_t *d_digests, unsigned log_leaves, unsigned cap_height,
                           const uint64_t *d_idx, size_t m, uint64_t *d_out);
/* fri_proof_of_work (fri/prover.rs:153-202), deterministic: returns the SMALLEST valid witness
 * (the reference's rayon find_any returns an arbitrary valid one), observes it and draws the
 * response like the reference does.  The candidates go through the challenger's permutation (Poseidon or KeccakPermutation). */
int p2hot_fri_pow(p2hot_ctx *ctx, p2hot_challenger *challenger, unsigned pow_bits, uint64_t *witness_out);
/* fri_committed_trees (fri/prover.rs:84-150) for M final polynomials of ONE shape in one set of launches: the M-form of
 * p2hot_fri_commit_dev.  Per round the M codewords are the 2M columns of one coset LDE (prover.rs:119, fri/oracle.rs:215-220), the
 * M round trees one forest of M << cap_height cap subtrees (prover.rs:99-104: proof j's digests and cap are contiguous and in the
 * single tree's layout), and one launch observes cap j and draws beta j for every transcript (prover.rs:106-109), one folds
 * (prover.rs:111-118).  The dummy caps of max_num_query_steps, the final polynomials and the zero padding to final_poly_coeff_len
 * (prover.rs:122-147) are observed by every transcript in one launch each.
 *   d_coeffs_planar  DEVICE planes [2][M][n]: component c of proof j's coefficients at (c * M + j) * n
 *   challengers      M distinct Poseidon transcripts of this context; transcript j is advanced exactly as p2hot_fri_commit_dev
 *                    advances it for proof j alone (the transcripts may hold different numbers of buffered elements)
 *   outputs (any may be NULL) are PROOF-MAJOR: proof j's block is what p2hot_fri_commit_dev writes for it, the blocks back to back
 *     d_leaves_out   DEVICE [M][leaf words], digests_out DEVICE (digests_on_device != 0) or host [M][digest words],
 *     caps_out       host [M][n_rounds][4 << cap_height], betas_out host [M][n_rounds][2], final_out host [M][n_final][2]
 * Every word equals M p2hot_fri_commit_dev calls'.  A call is split into groups of proofs so that the round scratch stays bounded
 * (M_group << (log_n + rate_bits) <= 2^22 extension elements; P2HOT_MANY_GROUP, read per call, lowers the proofs per group).
 * A Keccak transcript is P2HOT_EUNSUPPORTED (one at a time: p2hot_fri_commit_dev); everything is validated before the first enqueue. */
int p2hot_fri_commit_many_dev(p2hot_ctx *ctx, size_t M, const uint64_t *d_coeffs_planar, unsigned log_n, unsigned rate_bits,
                              unsigned cap_height, const unsigned *arity_bits, unsigned n_rounds, unsigned max_num_query_steps,
                              size_t final_poly_coeff_len, p2hot_challenger *const *challengers, uint64_t *d_leaves_out,
                              uint64_t *digests_out, int digests_on_device, uint64_t *caps_out, uint64_t *betas_out,
                              uint64_t *final_out);
/* fri_proof_of_work (fri/prover.rs:153-202) for M transcripts in one set of launches: the M-form of p2hot_fri_pow.  The candidate
 * chunks are shared by all proofs (grid: blocks x M) and a block of proof j retires at once when witness j is known; witnesses_out[j]
 * is the SMALLEST valid witness of transcript j, which then observes it and draws the response (prover.rs:197-198), as
 * p2hot_fri_pow does.  A transcript whose device-searched range holds no witness continues alone with host-checked chunks.
 * Keccak transcripts: P2HOT_EUNSUPPORTED. */
int p2hot_fri_pow_many(p2hot_ctx *ctx, size_t M, p2hot_challenger *const *challengers, unsigned pow_bits, uint64_t *witnesses_out);

/* ================================================================ prover session (HOST pointers)
 * What the patched plonky2 crate calls from the prover's main thread with ordinary Vec<F> buffers.  Everything between
 * the calls stays on the GPU behind opaque handles:
 *   p2hot_batch       a device-resident PolynomialBatch (fri/oracle.rs:30-37): polynomials (coefficients), the LDE
 *                     matrix = merkle_tree.leaves, merkle_tree.digests; optionally the input values
 *   p2hot_cols        a device-resident Vec<PolynomialValues> / Vec<PolynomialCoeffs> ([W][n]) that never visits the host
 *   p2hot_challenger  the Fiat-Shamir transcript (above)
 * A context runs ONE host-pointer call at a time; a second thread entering gets P2HOT_EBUSY (plonky2 calls these
 * from the main thread, outside its rayon closures).  Serialised by the library (busy guard): p2hot_commit*, p2hot_cols_upload,
 * p2hot_batch_coeffs / _rows / _paths / _digests / _subgroup_values, p2hot_eval_openings, p2hot_prove_openings, p2hot_partial_products,
 * p2hot_quotient_chunks, p2hot_quotient_polys, p2hot_quotient_polys_lookup, p2hot_lookup_polys, p2hot_cols_concat, p2hot_gate_sums,
 * p2hot_quotient_polys_gates, p2hot_quotient_polys_lookup_gates, p2hot_stark_lookup_polys, p2hot_stark_ctl_polys,
 * p2hot_stark_quotient_polys, p2hot_stark_constraint_accs, p2hot_stark_quotient_polys_air, p2hot_gate_sums_programs,
 * p2hot_quotient_polys_gate_programs, p2hot_quotient_polys_lookup_gate_programs, p2hot_ctx_trim, p2hot_batch_oracle_commit,
 * p2hot_batch_oracle_coeffs / _rows / _paths / _digests, p2hot_batch_prove_openings, p2hot_partial_products_many,
 * p2hot_commit_cols_many, p2hot_quotient_polys_gates_many, p2hot_eval_openings_many.  p2hot_batch_free / p2hot_batch_oracle_free / p2hot_cols_free may be called from any thread at any time (a
 * Drop, a finaliser): the block cache has its own lock.  Everything else -- the *_dev building blocks, p2hot_fri_commit,
 * p2hot_fri_pow, p2hot_challenger_* -- enqueues on the context's stream without a guard: the CALLER serialises those with
 * each other and with the host-pointer calls of the same context (the Rust shim holds the context behind a Mutex). */
#define P2HOT_EBUSY 5        /* another host-pointer call is running on this context */
#define P2HOT_ECOMM 6        /* collective (RCCL / caller-supplied transport) failure in the multi-GPU mode */
#define P2HOT_KEEP_VALUES 1u /* from_values: keep the input values on the device (p2hot_batch_values) */
/* p2hot_commit / _salted / _cols: `coeffs_out` is a TABLE of W host pointers (cast from `uint64_t *const *`), polynomial c's
 * n coefficients go to table[c] -- the caller's `polynomials: Vec<PolynomialCoeffs<F>>` (fri/oracle.rs:32) is W separate
 * vectors, and with this flag each is filled in place instead of being split out of one flat block afterwards */
#define P2HOT_COEFFS_PER_COLUMN 2u
/* p2hot_commit / _salted with leaves_out AND handle_out: the call returns when the cap, the coefficients and the digests are back;
 * the row-major leaf matrix (9.1 GB at the C3 wires shape: 3 x the rest of the call over PCIe) keeps travelling into leaves_out on
 * the context's leaf-copy stream, in min(64, N / 1024) consecutive row blocks (p2hot_batch_leaves_block_rows), first block first.  A row may be READ only after
 * p2hot_batch_leaves_wait(handle, row_lo, row_hi) covered it; the buffer may be FREED only after p2hot_batch_free(handle) (which
 * waits for the copy) or a wait over all rows.  leaves_out should be pinned (p2hot_host_alloc): a pageable destination makes the
 * copy a synchronous one.  The next commitments, the partial products and the quotient run beside the copy. */
#define P2HOT_LEAVES_ASYNC 4u
/* leaves_out in NATURAL LDE order instead of the committed order: leaves_out[i] = merkle_tree.leaves[reverse_bits(i, log2 N)], i.e.
 * `transpose(lde_values)` without the `reverse_index_bits_in_place` of fri/oracle.rs:97-98.  get_lde_values(i, step) (oracle.rs:142-147)
 * is then row i * step of the buffer, so the quotient loop of plonk/prover.rs:712-722 walks the buffer FORWARD -- the order the
 * P2HOT_LEAVES_ASYNC blocks arrive in -- and MerkleTree::get(r) is row reverse_bits(r).  p2hot_batch_rows / _paths and the proofs keep
 * the committed indexing: only the host copy's row order changes. */
#define P2HOT_LEAVES_NATURAL 8u
/* p2hot_commit / _salted / _cols: the Merkle tree's hasher in bits 8..15 of the flag word.  0 = PoseidonHash; n = 1..32 =
 * KeccakHash<n> (digests in 32-byte slots, see p2hot_keccak_merkle_dev); 33..255 is P2HOT_EINVAL.  The batch records its hasher:
 * p2hot_prove_openings opens Keccak batches with a Keccak challenger of the same n (see there); _many and the multi-GPU entry
 * points refuse them with P2HOT_EUNSUPPORTED;
 * p2hot_batch_rows / _paths / _digests / _coeffs, p2hot_eval_openings and p2hot_quotient_polys do not depend on the hasher. */
#define P2HOT_HASH_KECCAK(n) ((unsigned)(n) << 8)
#define P2HOT_HASH_MASK 0xFF00u

typedef struct p2hot_batch p2hot_batch;
typedef struct p2hot_cols p2hot_cols;

/* from_values (is_values != 0, fri/oracle.rs:57-79) / from_coeffs (:82-112), blinding = false.
 * cols: W host pointers to n = 2^log_n words each (Vec<PolynomialValues<F>> / Vec<PolynomialCoeffs<F>>).
 * coeffs_out [W][n], leaves_out [N][W], digests_out, cap_out: caller-allocated or NULL (anything not asked for is not
 * copied back: the leaf matrix is 9 GB at the C3 shape, and the query phase needs only a few dozen rows and paths).
 * handle_out (optional): the device-resident batch for p2hot_batch_rows / _paths / _coeffs, p2hot_eval_openings and
 * p2hot_prove_openings; free with p2hot_batch_free.  flags: P2HOT_KEEP_VALUES, P2HOT_COEFFS_PER_COLUMN, P2HOT_LEAVES_ASYNC,
 * P2HOT_LEAVES_NATURAL.
 * W = 0 is P2HOT_EINVAL for every commit entry point (the reference panics on polynomials[0], fri/oracle.rs:90). */
int p2hot_commit(p2hot_ctx *ctx, const uint64_t *const *cols, size_t W, unsigned log_n, unsigned rate_bits,
                 unsigned cap_height, int is_values, unsigned flags, uint64_t *coeffs_out, uint64_t *leaves_out,
                 uint64_t *digests_out, uint64_t *cap_out, p2hot_batch **handle_out);
/* the same with blinding = true (fri/oracle.rs:123-137; standard_recursion_zk_config, circuit_data.rs:135-137): the
 * reference appends SALT_SIZE = 4 random LDE-value vectors of length N to the leaves.  The random numbers stay the
 * caller's (Rust draws them with F::rand_vec / OsRng and hands them over): salt_cols = n_salt host pointers to N words
 * each, in the order F::rand_vec produced them (natural index, like the LDE values before transpose +
 * reverse_index_bits, oracle.rs:97-98).  Leaves are W + n_salt wide: leaves_out [N][W + n_salt], p2hot_batch_rows and
 * the opened rows of p2hot_prove_openings carry the salts (MerkleTree::get does; get_lde_values strips them, :146);
 * p2hot_batch_width stays W (the polynomials), p2hot_batch_leaf_width is W + n_salt.  n_salt = 0 is p2hot_commit. */
int p2hot_commit_salted(p2hot_ctx *ctx, const uint64_t *const *cols, size_t W, unsigned log_n, unsigned rate_bits,
                        unsigned cap_height, int is_values, unsigned flags, const uint64_t *const *salt_cols, size_t n_salt,
                        uint64_t *coeffs_out, uint64_t *leaves_out, uint64_t *digests_out, uint64_t *cap_out,
                        p2hot_batch **handle_out);
/* the same on a device-resident column set (the output of p2hot_partial_products / p2hot_quotient_chunks, or an upload).
 * CONSUMES `cols` -- its block becomes the batch's coefficients or kept values, or is released -- on success and on failure,
 * except for the failures detected before the set is touched: P2HOT_EBUSY and EVERY P2HOT_EINVAL (a null set, a set of
 * another context, a borrowed view (p2hot_batch_values), an empty set, a bad rate / cap height / flag word: all arguments are
 * validated first).  After those two codes the caller still owns the handle. */
int p2hot_commit_cols(p2hot_ctx *ctx, p2hot_cols *cols, unsigned rate_bits, unsigned cap_height, int is_values,
                      unsigned flags, uint64_t *coeffs_out, uint64_t *leaves_out, uint64_t *digests_out, uint64_t *cap_out,
                      p2hot_batch **handle_out);
/* M commitments of ONE shape in one set of launches (recursion workloads: the 2^12-row proofs of bench_recursion's chain,
 * examples/bench_recursion.rs:317-345, are latency-bound one at a time).  M is a power of two, W * M <= 65535.
 * Results equal M separate p2hot_commit calls (fri/oracle.rs:57-112 per proof), bit for bit.
 * cols[m * W + e]: column e of proof m (n words).  coeffs_out [M][W][n], digests_out [M][p2hot_num_digests][4],
 * caps_out [M][2^cap_height][4], each optional.  handles_out [M] (optional): one p2hot_batch per proof (rows, paths,
 * coefficients, p2hot_eval_openings, p2hot_prove_openings); the proofs share their device blocks, which return to the
 * context's cache when the last of the M handles is freed. */
int p2hot_commit_many(p2hot_ctx *ctx, const uint64_t *const *cols, size_t M, size_t W, unsigned log_n, unsigned rate_bits,
                      unsigned cap_height, int is_values, uint64_t *coeffs_out, uint64_t *digests_out, uint64_t *caps_out,
                      p2hot_batch **handles_out);
/* the device-pointer form: d_cols [W][M][n] (column e of every proof, then column e + 1, ...; becomes the coefficients in
 * place), d_lde [W][M][N] in the same interleaving, d_digests [M][num_digests][4], d_cap [M][2^cap_height][4]. */
int p2hot_commit_many_dev(p2hot_ctx *ctx, uint64_t *d_cols, size_t M, size_t W, unsigned log_n, unsigned rate_bits,
                          unsigned cap_height, int is_values, uint64_t *d_lde, uint64_t *d_digests, uint64_t *d_cap);
/* a handle over device buffers the CALLER owns (the outputs of p2hot_commit_dev): nothing is copied, p2hot_batch_free
 * frees only the handle.  d_coeffs [W][n] stride n, d_lde [W][N] stride N, d_digests the full tree's array. */
int p2hot_batch_wrap_dev(p2hot_ctx *ctx, const uint64_t *d_coeffs, const uint64_t *d_lde, const uint64_t *d_digests, size_t W,
                         unsigned log_n, unsigned rate_bits, unsigned cap_height, p2hot_batch **out);
size_t p2hot_batch_width(const p2hot_batch *batch);      /* polynomials */
size_t p2hot_batch_leaf_width(const p2hot_batch *batch); /* words per leaf: polynomials + salt columns */
unsigned p2hot_batch_degree_log(const p2hot_batch *batch);
/* `polynomials[first .. first + count)` (fri/oracle.rs:32), canonical: out [count][n] */
int p2hot_batch_coeffs(p2hot_batch *batch, size_t first, size_t count, uint64_t *out);
/* MerkleTree::get for m leaf indices (merkle_tree.rs:227): out [m][p2hot_batch_leaf_width] */
int p2hot_batch_rows(p2hot_batch *batch, const uint64_t *row_idx, size_t m, uint64_t *out);
/* merkle_tree_prove (merkle_tree.rs:151-190) for m leaf indices from the batch's device-resident digests:
 * out [m][log2(N) - cap_height][4].  With it the caller may pass digests_out = NULL to p2hot_commit and never copy
 * the digest array (0.54 GB at the C3 shape) to the host. */
int p2hot_batch_paths(p2hot_batch *batch, const uint64_t *leaf_idx, size_t m, uint64_t *out);
/* merkle_tree.digests (reference layout, hash/merkle_tree.rs:50-57): out [p2hot_num_digests(log2 N, cap_height)][4] */
int p2hot_batch_digests(p2hot_batch *batch, uint64_t *out);
/* P2HOT_LEAVES_ASYNC: blocks until rows [row_lo, row_hi) of the caller's leaves_out (in ITS row order: natural with
 * P2HOT_LEAVES_NATURAL, committed otherwise) have landed.  A batch without a pending copy returns at once; row_hi beyond the
 * leaf count or row_lo > row_hi is EINVAL.  This is the fence behind MerkleTree::get (hash/merkle_tree.rs:227) in the Rust shim. */
int p2hot_batch_leaves_wait(p2hot_batch *batch, size_t row_lo, size_t row_hi);
/* rows per block of the pending copy: min(64, N / 1024) blocks (at least one), delivered in order -- once row r has landed, so has
 * every row below (r / block_rows + 1) * block_rows, which is what a reader walking forward raises its "landed" mark to instead of
 * asking once per row (integration/p2hot.rs DeviceTree::fence).  0 when the batch has no copy in flight.  Lock-free like the wait,
 * and like it never writes p2hot_last_error: both may run beside a locked call of the same context. */
size_t p2hot_batch_leaves_block_rows(const p2hot_batch *batch);
/* the kept input values (P2HOT_KEEP_VALUES) as a BORROWED column set: valid while the batch lives; p2hot_cols_free on
 * the view leaves the batch's memory alone */
int p2hot_batch_values(p2hot_batch *batch, p2hot_cols **out);
/* polynomials [first, first + count) of the batch as values on the subgroup H_n, as an OWNED column set (free with
 * p2hot_cols_free): a forward NTT (field/src/fft.rs:53-65) of a copy of their device-resident coefficients.  For the sigma range
 * of the constants_sigmas commitment this is `prover_data.sigmas` (plonk/prover.rs:413) column-major: the `sigmas` input of
 * p2hot_partial_products, with no host transpose and no upload.  count == 0 or a range beyond the batch is EINVAL. */
int p2hot_batch_subgroup_values(p2hot_batch *batch, size_t first, size_t count, p2hot_cols **out);
/* returns the batch's device blocks to its context's block cache; call it BEFORE p2hot_ctx_destroy of that context
 * (the host-pointer entry points keep their device blocks in a per-context cache: a fresh allocation of the 9 GB LDE
 * matrix costs up to a second; p2hot_ctx_trim gives the cached free blocks back to the driver) */
void p2hot_batch_free(p2hot_batch *batch);
/* frees what the context only keeps for speed: the cached free device and pinned blocks (its helpers' too) and the per-size
 * L_0 denominator tables of p2hot_quotient_polys (8 bytes per point of the quotient coset; rebuilt on demand) */
int p2hot_ctx_trim(p2hot_ctx *ctx);
/* PINNED host memory from a grow-only cache of the context, for output buffers that live as long as a commitment -- above all the
 * flat leaf matrix (`leaves_out`, 9 GB at the C3 shape) the Rust shim keeps behind MerkleTree::get (hash/merkle_tree.rs:227).
 * A device-to-host copy into pinned memory runs at the PCIe rate and touches no fresh page; a fresh pageable allocation of that
 * size pays a page fault per 4 KiB while the copy runs, and a fresh PIN of that size costs seconds -- hence the cache: a block
 * released with p2hot_host_free (any thread, any time: a Drop) is handed out again by the next p2hot_host_alloc of a similar
 * size; p2hot_ctx_trim and p2hot_ctx_destroy give the cached blocks back to the OS.  Free every block before destroying the context. */
int p2hot_host_alloc(p2hot_ctx *ctx, size_t bytes, void **out);
void p2hot_host_free(p2hot_ctx *ctx, void *p);

/* device-resident column sets */
int p2hot_cols_upload(p2hot_ctx *ctx, const uint64_t *const *cols, size_t W, unsigned log_n, p2hot_cols **out);
int p2hot_cols_download(p2hot_cols *cols, size_t first, size_t count, uint64_t *out /* [count][n] */);
size_t p2hot_cols_width(const p2hot_cols *cols);
unsigned p2hot_cols_degree_log(const p2hot_cols *cols);
void p2hot_cols_free(p2hot_cols *cols);

/* OpeningSet::new (plonky2/src/plonk/proof.rs:314-327; starky/src/proof.rs StarkOpeningSet): every polynomial of every
 * listed batch at each extension point.  points [n_points][2].  out: for batch b in order, [n_points][W_b][2], concatenated. */
int p2hot_eval_openings(p2hot_ctx *ctx, const p2hot_batch *const *batches, size_t n_batches, const uint64_t *points,
                        size_t n_points, uint64_t *out);

/* FriBatchInfo (fri/structure.rs): an opening point and the polynomials opened there as (oracle_index, polynomial_index) */
typedef struct {
    uint64_t point[2];
    const uint32_t *oracle_index;
    const uint32_t *poly_index;
    size_t n_polys;
} p2hot_fri_batch_info;
/* FriParams / FriConfig (fri/mod.rs:19-60, :62-104) + the two Option<usize> of prove_openings (0 = None) */
typedef struct {
    unsigned rate_bits, cap_height, proof_of_work_bits, num_query_rounds;
    const unsigned *reduction_arity_bits;
    unsigned n_reduction_rounds;
    int hiding;                     /* FriParams::hiding: carried for the caller's transcript (fri/mod.rs:148); the prover's FRI path does not depend on it */
    unsigned max_num_query_steps;   /* fri/prover.rs:90 */
    size_t final_poly_coeff_len;    /* fri/prover.rs:89 */
} p2hot_fri_params;
/* FriProof (fri/proof.rs:95-110) as flat caller-allocated buffers; Q = num_query_rounds, R = rounds, m_0 = N,
 * m_{r+1} = m_r >> arity_bits[r]:
 *   commit_phase_merkle_caps [R][2^cap_height][4]
 *   final_poly               [m_R >> rate_bits][2]
 *   pow_witness
 *   query_indices            [Q] x_index of every query round (optional, may be NULL; the verifier re-derives them)
 *   query_round_proofs[q].initial_trees_proof.evals_proofs[o] = (leaf, path):
 *     initial_leaves         [Q][sum_o leaf_width_o]   the opened row (salts included) of every oracle, oracles in order
 *     initial_paths          [Q][n_oracles][log2(N) - cap_height][4]
 *   query_round_proofs[q].steps[r] = (evals, merkle_proof):
 *     step_evals             [Q][sum_r 2 * 2^arity_bits[r]]       evals of round r = 2^arity_bits[r] extension elements
 *     step_paths             [Q][sum_r (log2(m_r) - arity_bits[r] - cap_height) * 4] */
typedef struct {
    uint64_t *commit_phase_merkle_caps;
    uint64_t *final_poly;
    uint64_t pow_witness;
    uint64_t *query_indices;
    uint64_t *initial_leaves;
    uint64_t *initial_paths;
    uint64_t *step_evals;
    uint64_t *step_paths;
} p2hot_fri_proof;
typedef struct {
    size_t caps_words, final_poly_words, initial_leaves_words, initial_paths_words, step_evals_words, step_paths_words;
} p2hot_fri_proof_layout;
int p2hot_fri_proof_sizes(const p2hot_batch *const *oracles, size_t n_oracles, const p2hot_fri_params *params,
                          p2hot_fri_proof_layout *out);
/* PolynomialBatch::prove_openings (fri/oracle.rs:176-237) + fri_proof (fri/prover.rs:24-82): alpha, final_poly =
 * sum_i alpha^(k_i) (F_i - F_i(z_i)) / (X - z_i), its LDE, the commit phase (fri_committed_trees, :84-150), the
 * proof-of-work grind (:153-202, smallest witness) and the query rounds (:204-258), with the transcript advanced exactly
 * like the reference.  All oracles must share degree, rate and cap height.
 * The hasher is the config's (Challenger<F, C::Hasher>): either a Poseidon challenger and Poseidon oracles, or a KeccakHash<n>
 * challenger (p2hot_challenger_create_keccak) and KeccakHash<n> oracles (P2HOT_HASH_KECCAK(n)) of the same n -- then the round
 * trees, the transcript and the grind are Keccak, and digests / path entries are the 32-byte slots, bytes n..32 zero.  Any mixture
 * (Poseidon challenger with a Keccak oracle, Keccak challenger with a Poseidon oracle, different n) is P2HOT_EUNSUPPORTED before
 * anything is enqueued.  p2hot_prove_openings_many, p2hot_group_prove_openings and the sharded commits stay Poseidon-only: a Keccak
 * challenger or oracle there is P2HOT_EUNSUPPORTED. */
int p2hot_prove_openings(p2hot_ctx *ctx, const p2hot_fri_batch_info *batches, size_t n_batches,
                         const p2hot_batch *const *oracles, size_t n_oracles, p2hot_challenger *challenger,
                         const p2hot_fri_params *params, p2hot_fri_proof *proof);
/* M independent opening proofs per call (recursion workloads: many 2^12-row proofs, each a latency-bound chain of small
 * launches).  Proof j opens oracles[j * n_oracles .. + n_oracles) (handles of THIS context, e.g. from p2hot_commit_many) at
 * batches[j][0 .. n_batches[j]) with transcript challengers[j] and fills proofs[j]; every proof is computed exactly as by
 * p2hot_prove_openings (same buffers, same transcript afterwards).  Two paths, equal byte for byte:
 *   fused         Proofs of ONE SHAPE share every launch, on the caller's context and stream, with no helper threads: alpha_j and the
 *                 final polynomials (fri/oracle.rs:186-213) as planes [2][M][n], the commit phase as p2hot_fri_commit_many_dev runs
 *                 it (fri/prover.rs:84-150: per round one LDE of 2M columns, one forest, one transcript launch, one fold), the grind
 *                 as p2hot_fri_pow_many (prover.rs:153-202), then the query rounds (prover.rs:204-258) of the M oracles of each oracle
 *                 position and of the M round trees of each round, written in the proof layout above into one staging block that
 *                 one copy brings back.  Everything is validated before the first enqueue (a per-proof message names the proof)
 *                 and the call synchronises once.  A call is split into groups of proofs (p2hot_fri_commit_many_dev's bound).  A proof
 *                 whose device-searched grind range held no witness gets its transcript back and is proved again alone.
 *                 One shape: distinct transcripts; the same n_batches[j]; the same (oracle_index, poly_index) lists in every batch
 *                 (the points are per proof); the same polynomial and salt widths per oracle position.  The handles may be shares of
 *                 one p2hot_commit_many block or separately committed, in any mixture.
 *   side by side  Anything else, and every call under P2HOT_MANY_FUSED=0 (read per call): up to 4 sibling contexts of the same GPU --
 *                 own streams, driven by their own host threads -- run M single-proof chains concurrently.
 * Measured at the recursion shape the fused path wins from M = 1 on, so every eligible call takes it.
 * Keccak transcripts or oracles: P2HOT_EUNSUPPORTED on both paths. */
int p2hot_prove_openings_many(p2hot_ctx *ctx, size_t M, const p2hot_fri_batch_info *const *batches, const size_t *n_batches,
                              const p2hot_batch *const *oracles, size_t n_oracles, p2hot_challenger *const *challengers,
                              const p2hot_fri_params *fp, p2hot_fri_proof *proofs);

/* all_wires_permutation_partial_products (plonk/prover.rs:356-449) on device-resident columns: wires = columns
 * [wires_first_col, +num_routed) of `wires` (e.g. p2hot_batch_values of the wires commitment), sigmas likewise (the
 * constants_sigmas commitment's values: sigma_j(w_n^i)).  k_is HOST [num_routed], betas / gammas HOST [num_challenges],
 * degree = quotient_degree_factor.  Output rows ordered as the prover commits them (prover.rs:224-229): Z of challenge
 * 0 .. nc-1, then the partial products of challenge 0, 1, ...: out_host [nc * (num_prods + 1)][n] and / or out_cols
 * (feed it to p2hot_commit_cols(is_values = 1)); either may be NULL. */
int p2hot_partial_products(p2hot_ctx *ctx, const p2hot_cols *wires, size_t wires_first_col, const p2hot_cols *sigmas,
                           size_t sigmas_first_col, const uint64_t *k_is, unsigned num_routed, unsigned degree,
                           const uint64_t *betas, const uint64_t *gammas, unsigned num_challenges, uint64_t *out_host,
                           p2hot_cols **out_cols);
/* The gate-independent tail of compute_quotient_polys (plonk/prover.rs:274-289, :810-815): quotient_values[c] are the
 * values of challenge c's quotient on the coset g*H of size n << ceil(log2(quotient_degree_factor)) (natural order);
 * coset_ifft, trim to quotient_degree_factor * n coefficients (P2HOT_EINVAL "Quotient has failed ..." if the tail is
 * not zero, where the reference panics) and split into chunks of n: chunks_out = [nc * quotient_degree_factor][n]
 * coefficients, ready for p2hot_commit_cols(is_values = 0). */
int p2hot_quotient_chunks(p2hot_ctx *ctx, const uint64_t *const *quotient_values, unsigned num_challenges,
                          unsigned degree_bits, unsigned quotient_degree_factor, p2hot_cols **chunks_out);
/* compute_quotient_polys (plonk/prover.rs:609-815) WITHOUT its gate evaluation: the permutation argument's share of
 * eval_vanishing_poly_base_batch (plonk/vanishing_poly.rs:167-330) evaluated on the quotient coset from the device-resident LDE
 * matrices of the three commitments -- for every x = g * w^i of the coset of size n << log2_ceil(quotient_degree_factor):
 *   terms  L_0(x) (Z_c(x) - 1)  for every challenge c, then check_partial_products (util/partial_products.rs:52-79) per challenge:
 *          prev_acc * prod(wire_j + beta_c k_j x + gamma_c) - next_acc * prod(wire_j + beta_c sigma_j(x) + gamma_c) per chunk of
 *          quotient_degree_factor routed wires, accumulators Z_c(x), the partial products, Z_c(g x);
 *   value_a(x) = (reduce_with_powers(terms, alpha_a) + alpha_a^K * gate_sums[a][i]) / Z_H(x),  K = the number of terms above
 * -- the gate constraint terms (circuit specific, out of scope) are the CALLER's: gate_sums[a] = their own reduce_with_powers
 * by alpha_a on the same coset (n << qbits words, natural order), or gate_sums = NULL for none --, followed by the tail of
 * p2hot_quotient_chunks (coset_ifft, the divisibility check, chunks of n coefficients).
 *   wires, constants_sigmas, zs_partial_products: commitments of THIS context with the same degree and rate; the routed wires are
 *     columns 0 .. num_routed of `wires`, the sigma polynomials columns sigmas_first_col .. of `constants_sigmas`
 *     (common_data.sigmas_range()), `zs_partial_products` holds Z_0 .. Z_{nc-1} then the partial products of challenge 0, 1, ...
 *     (prover.rs:224-229: the order p2hot_partial_products emits)
 *   k_is HOST [num_routed]; betas / gammas / alphas HOST [num_challenges], 1 <= num_challenges <= 4
 *   values_out (optional) HOST [num_challenges][n << qbits]: the quotient VALUES on the coset (prover.rs:805: quotient_values)
 *   chunks_out (optional): [num_challenges * quotient_degree_factor][n] coefficients for p2hot_commit_cols(is_values = 0)
 * P2HOT_EINVAL "Quotient has failed ..." when the result is not a polynomial of the expected degree (the reference panics). */
int p2hot_quotient_polys(p2hot_ctx *ctx, const p2hot_batch *wires, const p2hot_batch *constants_sigmas, size_t sigmas_first_col,
                         const p2hot_batch *zs_partial_products, const uint64_t *k_is, unsigned num_routed,
                         unsigned quotient_degree_factor, const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas,
                         unsigned num_challenges, const uint64_t *const *gate_sums, uint64_t *values_out, p2hot_cols **chunks_out);

/* ---------------------------------------------------------------- the lookup argument (circuits with lookup tables)
 * Poseidon configuration, single GPU: a KeccakHash commitment is P2HOT_EUNSUPPORTED, and the multi-GPU group has no lookup entry point.
 * Slots: num_lu_slots = LookupGate::num_slots = num_routed_wires / 2 (gates/lookup.rs:58-69: looking inp / out on wires 2s, 2s + 1),
 * num_lut_slots = LookupTableGate::num_slots = num_routed_wires / 3 (gates/lookup_table.rs:64-82: looked inp / out / multiplicity on
 * wires 3s, 3s + 1, 3s + 2).  deltas HOST [num_challenges][4] = ChallengeA, ChallengeB, ChallengeAlpha, ChallengeDelta
 * (plonk/circuit_builder.rs:68-73), the order of the prover's `deltas`.
 *
 * compute_all_lookup_polys (plonk/prover.rs:451-605): for every challenge RE and the S = ceil(num_lu_slots / lookup_degree) partial
 * SLDC polynomials as values on the trace subgroup (lookup_degree = max_quotient_degree_factor - 1, prover.rs:470-473); rows outside
 * every [last_lu_gate, first_lut_gate] are zero.
 *   wires        columns [wires_first_col, ...) of a device-resident column set: MatrixWitness.wire_values
 *   lookup_rows  HOST [num_luts][3] = last_lu_gate, last_lut_gate, first_lut_gate (LookupWire), in prover_data.lookup_rows order.  The
 *                regions are processed in that order, each reading the values at first_lut_gate + 1 as the earlier ones left them
 *                (prover.rs:517, :528, :561)
 *   out_host [num_challenges * (S + 1)][n] and / or out_cols: RE, SLDC_0 .. SLDC_{S-1} of challenge 0, then challenge 1, ...
 * P2HOT_EINVAL: first_lut_gate + 1 >= n (the reference indexes out of bounds), rows not ordered last_lu <= last_lut <= first_lut, slots
 * beyond the wires given, lookup_degree == 0, num_challenges outside 1..4, and a zero alpha - combination ("Tried to invert zero":
 * the reference panics in batch_multiplicative_inverse). */
int p2hot_lookup_polys(p2hot_ctx *ctx, const p2hot_cols *wires, size_t wires_first_col, unsigned num_lu_slots, unsigned num_lut_slots,
                       unsigned lookup_degree, const uint64_t *lookup_rows, unsigned num_luts, const uint64_t *deltas,
                       unsigned num_challenges, uint64_t *out_host, p2hot_cols **out_cols);
/* p2hot_quotient_polys for a circuit with lookup tables: the terms of check_lookup_constraints_batch (plonk/vanishing_poly.rs:515-664)
 * of challenge 0, 1, ... enter the term list between the partial-product terms and the gate terms (vanishing_poly.rs:317-322):
 *   value_a(x) = (reduce_with_powers(permutation terms ++ lookup terms, alpha_a) + alpha_a^(K + Klu) * gate_sums[a][i]) / Z_H(x),
 *   Klu = num_challenges * (4 + num_luts + 2 S),  S = ceil(num_lu_slots / (quotient_degree_factor - 1))
 * Every argument of p2hot_quotient_polys keeps its meaning, and:
 *   zs_partial_products_lookups  Z_0 .. Z_{nc-1}, the partial products, then the lookup polynomials in p2hot_lookup_polys' order
 *                                (prover.rs:237-241): exactly nc (1 + num_prods) + nc (S + 1) polynomials, else P2HOT_EINVAL
 *   lookup_selectors_first_col   the 4 + num_luts lookup selector columns of constants_sigmas: TransSre, TransLdc, InitSre, LastLdc
 *                                (gates/selectors.rs:34-78), then one end selector per LUT (:82-99)
 *   lut_re_poly_evals            HOST [num_challenges][num_luts]: get_lut_poly(..).eval(delta) (prover.rs:652-680), the caller's
 * 2 num_lu_slots or 3 num_lut_slots beyond the wires commitment, and num_challenges outside 1..4, are P2HOT_EINVAL. */
int p2hot_quotient_polys_lookup(p2hot_ctx *ctx, const p2hot_batch *wires, const p2hot_batch *constants_sigmas, size_t sigmas_first_col,
                                const p2hot_batch *zs_partial_products_lookups, const uint64_t *k_is, unsigned num_routed,
                                unsigned quotient_degree_factor, const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas,
                                unsigned num_challenges, const uint64_t *const *gate_sums, unsigned num_lu_slots, unsigned num_lut_slots,
                                unsigned num_luts, size_t lookup_selectors_first_col, const uint64_t *deltas,
                                const uint64_t *lut_re_poly_evals, uint64_t *values_out, p2hot_cols **chunks_out);
/* a's columns followed by b's (same degree, same context) as a NEW owned set; a and b stay valid.  The Zs / partial products and the
 * lookup polynomials go into one commitment (prover.rs:237-241): concat, then p2hot_commit_cols(is_values = 1). */
int p2hot_cols_concat(p2hot_ctx *ctx, const p2hot_cols *a, const p2hot_cols *b, p2hot_cols **out);

/* ---------------------------------------------------------------- the standard gates' constraints (D = 2)
 * evaluate_gate_constraints_base_batch (plonk/vanishing_poly.rs:702-728) on the quotient coset for fourteen gates of the reference.
 * A gate of common_data.gates is described by
 *   kind            P2HOT_GATE_*
 *   row             its index in common_data.gates: the `row` compute_filter excludes (gates/gate.rs:326-333)
 *   selector_index  selectors_info.selector_indices[row]; [group_first, group_end) = selectors_info.groups[selector_index]
 *   param0          Constant: num_consts; Arithmetic / ArithmeticExtension / MulExtension: num_ops; BaseSum: num_limbs (<= 63)
 *   param1          BaseSum: the base B, 2 <= B <= quotient_degree_factor: the range constraint of a limb has degree B, and a
 *                   circuit holds a gate only if group size + degree <= quotient degree factor + 1 (gates/selectors.rs:101-160)
 * and the set adds num_selectors = selectors_info.num_selectors(), num_lookup_selectors (4 + num_luts, or 0) and the public inputs
 * hash.  At a point x_i the local wires / constants are row bitrev(i) of the wires / constants_sigmas commitments; with
 * s = constants[selector_index]
 *   filter_g = prod_{k in group, k != row} (k - s), times (0xFFFFFFFF - s) when num_selectors > 1      (gate.rs:326-333)
 * the gate's own local_constants[c] is constants column num_selectors + num_lookup_selectors + c (gate.rs:179), and since every
 * gate's constraints are added into one vector from index 0 (vanishing_poly.rs:722-725) and the reduction is linear
 *   gate_sums[a][i] = sum_g filter_g(x_i) sum_j alpha_a^j c_{g,j}(x_i)                                  (canonical)
 * Constraints c_{g,j}, in the reference's order:
 *   NOOP            none (gates/noop.rs)
 *   CONSTANT        constants[i] - wires[i], i < num_consts                                            (constant.rs:126-128)
 *   PUBLIC_INPUT    wires[i] - public_inputs_hash[i], i < 4                                            (public_input.rs:108-112)
 *   ARITHMETIC      w[4i+3] - (w[4i] w[4i+1] c0 + w[4i+2] c1)                                          (arithmetic_base.rs:173-184)
 *   ARITHMETIC_EXT  per op the two base components of out - ((m0 m1) c0 + addend c1) in F[X]/(X^2 - 7); m0, m1, addend, out on
 *                   wires 8i .. 8i+8                                                                   (arithmetic_extension.rs:92-110)
 *   MUL_EXT         per op the two components of out - (m0 m1) c0; m0, m1, out on wires 6i .. 6i+6     (multiplication_extension.rs:86-101)
 *   BASE_SUM        sum_k limb_k B^k - w[0], then per limb prod_{t < B} (limb - t); limbs on wires 1 ..  (base_sum.rs:153-170)
 *   POSEIDON        the 123 constraints over 135 wires of PoseidonGate (poseidon.rs:204-283): swap (swap - 1), four deltas, the
 *                   S-box inputs of full rounds 1..3, of the 22 partial rounds in their FAST form (hash/poseidon.rs:365-373,
 *                   :415-441, :516-542), of the second four full rounds, and the 12 outputs; the state continues from the wire
 *                   after every constrained S-box input
 * The six gates a recursive verifier circuit adds under standard_recursion_config (the second enum below, kinds 16..21; an
 * "extension element on wires c, c + 1" is c + (c + 1) X in F[X]/(X^2 - 7), and a constraint on one yields component 0, then 1):
 *   POSEIDON_MDS    out_k - MDS(inputs)_k, k < 12; input k on wires 2k, 2k + 1, output k on 24 + 2k, 24 + 2k + 1: 48 wires, 24
 *                   constraints                                                                         (poseidon_mds.rs:156-175)
 *   REDUCING        param0 = num_coeffs >= 1.  output on wires 0..2, alpha 2..4, old_acc 4..6, base-field coeffs 6 .. 6 + nc,
 *                   acc_k on 6 + nc + 2k for k < nc - 1, the last accumulator is the output; constraint pair k =
 *                   acc alpha + coeff_k - acc_k, then acc continues from the WIRE acc_k: 3 nc + 4 wires   (reducing.rs:107-127)
 *   REDUCING_EXT    the same with extension coeffs on 6 + 2k and the accumulators from 6 + 2 nc: 4 nc + 4 wires
 *                                                                                                       (reducing_extension.rs:109-128)
 *   RANDOM_ACCESS   param0 = num_copies >= 1, param1 = bits | num_extra_constants << 8, 1 <= bits <= 6, bits + 1 <=
 *                   quotient_degree_factor.  Copy c: access_index on wire s c, claimed element s c + 1, the 2^bits list items from
 *                   s c + 2 (s = 2 + 2^bits); its bits on s copies + extra + c bits + l.  Per copy b (b - 1) per bit, the bits
 *                   folded big endian (acc + acc + b) minus access_index, the list folded pairwise x + b (y - x), bit 0 first,
 *                   minus claimed; then constants[k] - wires[s copies + k], k < extra                    (random_access.rs:302-343)
 *   EXPONENTIATION  param0 = num_power_bits >= 1, quotient_degree_factor >= 4.  base on wire 0, little-endian power bits 1 .. 1 + n,
 *                   output 1 + n, intermediates from 2 + n; constraint k = prev (bit base + 1 - bit) - inter_k with prev = 1 or
 *                   inter_{k-1}^2 and bit = power_bits[n - 1 - k]; last output - inter_{n-1}             (exponentiation.rs:210-243)
 *   COSET_INTERPOLATION  param0 = subgroup_bits 1..5 (N = 2^subgroup_bits points), param1 = degree d, 2 <= d <= N, d <=
 *                   quotient_degree_factor; ni = (N - 2) / (d - 1).  shift on wire 0, value k on 1 + 2k, evaluation point 1 + 2N,
 *                   evaluation value next, from 1 + 2N + 4 the ni intermediate evals, the ni intermediate prods, the shifted point.
 *                   point - shifted shift; the barycentric walk eval <- eval (x - x_k) + (w_k v_k) prod, prod <- prod (x - x_k)
 *                   from (0, 1) over the first d points of two_adic_subgroup(subgroup_bits); per intermediate inter_eval - eval,
 *                   inter_prod - prod, and the walk goes on from the WIRES over the next d - 1 points (clipped at N); last
 *                   evaluation_value - eval.  The library computes the domain and the weights w_k = x_k / N itself
 *                                                                                                       (coset_interpolation.rs:251-298, :553-580)
 * LookupGate / LookupTableGate have no constraints of their own; every other gate -- a user-defined one -- travels as a gate
 * program ("gate programs" below) or stays the caller's (the host gate_sums of the entry points below).  Kinds 8..15 and above 21
 * are P2HOT_EUNSUPPORTED. */
enum { P2HOT_GATE_NOOP, P2HOT_GATE_CONSTANT, P2HOT_GATE_PUBLIC_INPUT, P2HOT_GATE_ARITHMETIC,
       P2HOT_GATE_ARITHMETIC_EXT, P2HOT_GATE_MUL_EXT, P2HOT_GATE_BASE_SUM, P2HOT_GATE_POSEIDON };
enum { P2HOT_GATE_POSEIDON_MDS = 16, P2HOT_GATE_REDUCING, P2HOT_GATE_REDUCING_EXT, P2HOT_GATE_RANDOM_ACCESS,
       P2HOT_GATE_EXPONENTIATION, P2HOT_GATE_COSET_INTERPOLATION };
typedef struct p2hot_gate { uint32_t kind, row, selector_index, group_first, group_end, param0, param1; } p2hot_gate;
typedef struct p2hot_gate_set { const p2hot_gate *gates; uint32_t num_gates, num_selectors, num_lookup_selectors;
                                uint64_t public_inputs_hash[4]; } p2hot_gate_set;
/* The reduced gate sums alone: out_host HOST [num_challenges][n << log2_ceil(quotient_degree_factor)], natural order, canonical.
 * wires / constants_sigmas as in p2hot_quotient_polys (any hasher); sigmas_first_col bounds the constants a gate may read.
 * Raised before anything is enqueued -- P2HOT_EUNSUPPORTED: an unknown kind.  P2HOT_EINVAL: row outside its group (or a group of
 * more than 256 gates), selector_index >= num_selectors, selectors + lookup selectors + the constants a gate reads beyond
 * sigmas_first_col, a gate's wires beyond the wires commitment, B < 2, B > quotient_degree_factor or num_limbs > 63, a parameter of
 * the kinds 16..21 outside the range stated above or a degree above quotient_degree_factor, gates->gates null with num_gates > 0, a
 * null set, commitments of another context, degree or rate, num_challenges outside 1..4. */
int p2hot_gate_sums(p2hot_ctx *ctx, const p2hot_batch *wires, const p2hot_batch *constants_sigmas, size_t sigmas_first_col,
                    const p2hot_gate_set *gates, unsigned quotient_degree_factor, const uint64_t *alphas, unsigned num_challenges,
                    uint64_t *out_host);
/* p2hot_quotient_polys / p2hot_quotient_polys_lookup with the gates of `gates` evaluated on the device: every argument keeps its
 * meaning, and the host gate_sums (or NULL) is ADDED to the device-evaluated sums -- the residual of the gates the library does
 * not know, evaluated by the caller (eval_filtered_base_batch, gate.rs:158-185).  Launch order: the gate kernels, the lookup
 * kernel (if any) with their result as its gate sums, the permutation kernel.  Errors as p2hot_gate_sums and the extended entry
 * point, before anything is enqueued; *chunks_out is NULL on failure. */
int p2hot_quotient_polys_gates(p2hot_ctx *ctx, const p2hot_batch *wires, const p2hot_batch *constants_sigmas, size_t sigmas_first_col,
                               const p2hot_batch *zs_partial_products, const uint64_t *k_is, unsigned num_routed,
                               unsigned quotient_degree_factor, const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas,
                               unsigned num_challenges, const uint64_t *const *gate_sums, const p2hot_gate_set *gates,
                               uint64_t *values_out, p2hot_cols **chunks_out);
int p2hot_quotient_polys_lookup_gates(p2hot_ctx *ctx, const p2hot_batch *wires, const p2hot_batch *constants_sigmas, size_t sigmas_first_col,
                                      const p2hot_batch *zs_partial_products_lookups, const uint64_t *k_is, unsigned num_routed,
                                      unsigned quotient_degree_factor, const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas,
                                      unsigned num_challenges, const uint64_t *const *gate_sums, unsigned num_lu_slots, unsigned num_lut_slots,
                                      unsigned num_luts, size_t lookup_selectors_first_col, const uint64_t *deltas,
                                      const uint64_t *lut_re_poly_evals, const p2hot_gate_set *gates, uint64_t *values_out,
                                      p2hot_cols **chunks_out);

/* ================================================================ the middle of a proof for M witnesses of ONE circuit
 * p2hot_commit_many and p2hot_prove_openings_many batch the two ends of M recursion-size proofs (2^12 rows: every launch costs more
 * than its work).  The four entry points below batch what lies between them -- partial products and Zs, their commitment from
 * device columns, the quotient with its gate constraints, its commitment, the OpeningSet -- for M witnesses of one circuit:
 * sigmas, constants, selectors, the gate set and k_is are shared, wires, challenges and the public-inputs hash differ per proof.
 * Inputs: any M >= 1; the handles of the proofs need not come from one p2hot_commit_many (shares of one block and separately
 * committed batches mix freely; a per-proof device table carries base pointers, column strides, challenges and hash words to the
 * kernels, one grid row per proof).  Outputs: where a column set comes back it is ONE set in p2hot_commit_many_dev's interleaved
 * layout [W][M][n], column e of proof m being column e * M + m, ready for p2hot_commit_cols_many -- which inherits commit_many's
 * power-of-two M; for any other M take the host outputs or commit proof by proof.  Every result equals M single-proof calls bit for
 * bit (same canonical words, same order).  Everything is validated before the first enqueue (null entries, foreign contexts,
 * proofs of different degree or rate; a per-proof message names the proof), M == 0 is P2HOT_OK with nothing done, numeric
 * failures found on the device use one flag word per proof, and each call synchronises the host once.
 * NOT in the M-form, left to the single-proof entry points: the host gate_sums residual, lookups and gate programs; Keccak trees in
 * p2hot_commit_cols_many; the multi-GPU group.  (p2hot_prove_openings_many batches proofs of one shape in the same way.) */

/* all_wires_permutation_partial_products for M witnesses of one circuit.  wires[m]: the wires commitment of proof m (any
 * handle of this context, e.g. from p2hot_commit_many); the routed wires' VALUES on H are recomputed on the device from its
 * coefficients (forward NTT, as p2hot_batch_subgroup_values does), nothing is uploaded.  sigmas: ONE column set shared by
 * all proofs.  betas / gammas HOST [M][nc].  out_host [M][rows][n] (rows = nc * (num_prods + 1), p2hot_partial_products'
 * order) and / or out_cols: ONE set of rows * M columns in the interleaved layout.  A zero denominator in proof j is
 * P2HOT_EINVAL and the message names j.  num_challenges 1..4; M * num_routed <= 65535. */
int p2hot_partial_products_many(p2hot_ctx *ctx, size_t M, const p2hot_batch *const *wires, size_t wires_first_col,
                                const p2hot_cols *sigmas, size_t sigmas_first_col, const uint64_t *k_is, unsigned num_routed,
                                unsigned degree, const uint64_t *betas, const uint64_t *gammas, unsigned num_challenges,
                                uint64_t *out_host, p2hot_cols **out_cols);

/* p2hot_commit_cols for an interleaved set of W * M columns: p2hot_commit_many_dev on the set's block, M handles out
 * (shared blocks, freed with the last handle, as p2hot_commit_many's).  Poseidon trees; M a power of two, W * M <= 65535
 * (commit_many's limits, same messages).  Consumes `cols` under exactly p2hot_commit_cols' ownership rule: P2HOT_EINVAL and
 * P2HOT_EBUSY mean "not consumed", as does M == 0.  caps_out [M][2^cap_height][4], optional. */
int p2hot_commit_cols_many(p2hot_ctx *ctx, p2hot_cols *cols, size_t M, unsigned rate_bits, unsigned cap_height, int is_values,
                           uint64_t *caps_out, p2hot_batch **handles_out);

/* p2hot_quotient_polys_gates for M witnesses of one circuit: wires[m] / zs_partial_products[m] per proof, constants_sigmas
 * and the gate set shared; betas / gammas / alphas HOST [M][nc]; public_inputs_hashes HOST [M][4] (replaces the set's own
 * field per proof; NULL = the set's for all).  gates = NULL: permutation terms only.  values_out HOST [M][nc][n << qbits];
 * chunks_out: ONE set of nc * quotient_degree_factor * M columns, interleaved, ready for p2hot_commit_cols_many(is_values = 0).
 * "Quotient has failed ..." names the first proof whose tail is not zero. */
int p2hot_quotient_polys_gates_many(p2hot_ctx *ctx, size_t M, const p2hot_batch *const *wires, const p2hot_batch *constants_sigmas,
                                    size_t sigmas_first_col, const p2hot_batch *const *zs_partial_products, const uint64_t *k_is,
                                    unsigned num_routed, unsigned quotient_degree_factor, const uint64_t *betas, const uint64_t *gammas,
                                    const uint64_t *alphas, unsigned num_challenges, const p2hot_gate_set *gates,
                                    const uint64_t *public_inputs_hashes, uint64_t *values_out, p2hot_cols **chunks_out);

/* p2hot_eval_openings for M proofs: proof j evaluates batches[j * n_batches .. + n_batches) at points[j] ([n_points][2]);
 * the same handle may appear for several j (the shared constants_sigmas).  out: proof j's block in p2hot_eval_openings'
 * layout, the M blocks back to back. */
int p2hot_eval_openings_many(p2hot_ctx *ctx, size_t M, const p2hot_batch *const *batches, size_t n_batches,
                             const uint64_t *points, size_t n_points, uint64_t *out);

/* ================================================================ starky: logUp lookups and cross-table lookups of one STARK table
 * The stage of starky/src/prover.rs::prove_with_commitment between the trace commitment and the quotient commitment.  Poseidon
 * configuration, single GPU: a KeccakHash commitment is P2HOT_EUNSUPPORTED, and the multi-GPU group has no entry point here.
 *
 * Descriptors.  The reference's Column (starky/src/lookup.rs:137-141: current-row terms, next-row terms, a constant) and Filter
 * (lookup.rs:37-40: degree-2 products plus degree-1 constants) as flat HOST arrays the library uploads per call:
 *   term     coeff * trace[col] of the current row (next = 0) or of the next row (next = 1)
 *   column   terms [first_term, first_term + num_terms) plus `constant`
 *   filter   sum of column[products[2 p]] * column[products[2 p + 1]] over p in [first_product, + num_products), plus the sum of
 *            column[constants[k]] over k in [first_constant, + num_constants); Filter::default() is one constant-1 column
 *   lookup   Lookup (lookup.rs:415-429): looking columns [first_column, + num_columns), their filters [first_filter, + num_columns),
 *            the table column and the frequencies column (column ids)
 *   looking  one (columns, filter) of a CTL Z (cross_table_lookup.rs:155-167): columns [first_column, + num_columns), a filter id
 *   ctl_z    one CtlZData: looking entries [first_looking, + num_looking) and its GrandProductChallenge
 * Evaluation: Column::eval_table (lookup.rs:324-335; next row = (i + 1) mod n) when the polynomials are generated,
 * Column::eval_with_next (:306-321) for looking columns and filters in the quotient, Column::eval (:293-303, current-row terms
 * ONLY) for the table and frequencies columns in the quotient (lookup.rs:851, :856).
 * chunk = constraint_degree.checked_sub(1).unwrap_or(1) (lookup.rs:439, :670, :755); constraint_degree == 1 divides by zero in the
 * reference and is P2HOT_EINVAL.  eval_helper_columns knows chunks of one or two columns only (lookup.rs:675-691, `todo!`): a lookup
 * or a Z with a chunk of three or more is P2HOT_EUNSUPPORTED from all three entry points.
 * P2HOT_EINVAL from all three, before anything is enqueued: a term's col beyond the trace's width; a term, column, filter or
 * looking id beyond its array; a lookup with num_columns == 0 or a Z with num_looking == 0; num_challenges outside 1..4; null
 * arrays with a nonzero count.  A zero col + x, table + x or combined v ("Tried to invert zero": the reference panics in
 * batch_multiplicative_inverse) is P2HOT_EINVAL after the kernels ran. */
typedef struct p2hot_stark_term { uint32_t col, next; uint64_t coeff; } p2hot_stark_term;
typedef struct p2hot_stark_column { uint32_t first_term, num_terms; uint64_t constant; } p2hot_stark_column;
typedef struct p2hot_stark_filter { uint32_t first_product, num_products, first_constant, num_constants; } p2hot_stark_filter;
typedef struct p2hot_stark_lookup { uint32_t first_column, num_columns, first_filter, table_column, frequencies_column; } p2hot_stark_lookup;
typedef struct p2hot_stark_looking { uint32_t first_column, num_columns, filter; } p2hot_stark_looking;
typedef struct p2hot_stark_ctl_z { uint32_t first_looking, num_looking; uint64_t beta, gamma; } p2hot_stark_ctl_z;
typedef struct p2hot_stark_tables { const p2hot_stark_term *terms; const p2hot_stark_column *columns; const uint32_t *products;
                                    const uint32_t *constants; const p2hot_stark_filter *filters; const p2hot_stark_looking *looking;
                                    uint32_t num_terms, num_columns, num_products, num_constants, num_filters, num_looking; } p2hot_stark_tables;
/* lookup_helper_columns (starky/src/lookup.rs:579-652) for every lookup and every challenge, in the order of
 * starky/src/prover.rs:177-195: per lookup, per challenge x, the helper columns h_0 .. h_{H-1}, H = ceil(num_columns / chunk), then Z:
 *   h_k[i] = sum_{c in chunk k} filter_c(i) / (col_c(i) + x),  Z[0] = 0,  Z[i+1] = Z[i] + sum_k h_k[i] - freq(i) / (table(i) + x)
 * (1 / (table + x) is not an output column, whatever lookup.rs:433-436 says).
 *   trace       device-resident column set, 2^k rows
 *   challenges  HOST [num_challenges]
 *   out_host    [sum_l num_challenges (H_l + 1)][n] and / or out_cols (ready for p2hot_cols_concat / p2hot_commit_cols) */
int p2hot_stark_lookup_polys(p2hot_ctx *ctx, const p2hot_cols *trace, const p2hot_stark_tables *tables, const p2hot_stark_lookup *lookups,
                             unsigned num_lookups, const uint64_t *challenges, unsigned num_challenges, unsigned constraint_degree,
                             uint64_t *out_host, p2hot_cols **out_cols);
/* partial_sums (starky/src/cross_table_lookup.rs:383-414) for every CTL Z of one table, in get_ctl_auxiliary_polys' order
 * (cross_table_lookup.rs:253-261): the helper columns of all Zs in the order given, then all Zs.  For a Z with entries e:
 *   v_e(i) = sum_j col_{e,j}(i) beta^j + gamma (GrandProductChallenge::combine, lookup.rs:457-464),
 *   h_k = sum_{e in chunk k} filter_e / v_e,  Z[n-1] = sum_k h_k[n-1],  Z[i] = Z[i+1] + sum_k h_k[i]
 * and a Z with ONE entry has no helper column: its Z sums filter / v directly (cross_table_lookup.rs:407-411).
 *   zs_first    NULL or HOST [num_zs]: Z[0] of every Z (StarkOpeningSet::ctl_zs_first, starky/src/proof.rs)
 * Which Z belongs to which table (cross_table_lookup_data's group_by, cross_table_lookup.rs:270-339) is the caller's bookkeeping. */
int p2hot_stark_ctl_polys(p2hot_ctx *ctx, const p2hot_cols *trace, const p2hot_stark_tables *tables, const p2hot_stark_ctl_z *ctl_zs,
                          unsigned num_zs, unsigned constraint_degree, uint64_t *out_host, p2hot_cols **out_cols, uint64_t *zs_first);
/* compute_quotient_polys (starky/src/prover.rs:488-671) without Stark::eval_packed_generic: the terms of
 * eval_packed_lookups_generic (lookup.rs:804-863) and eval_cross_table_lookup_checks (cross_table_lookup.rs:558-629) at every
 * point x = g w^i of the coset of size n << qbits, qdf = max(1, constraint_degree - 1), qbits = log2_ceil(qdf) (prover.rs:516),
 * local row = get_lde_values(i, step), next row = index (i + 2^qbits) mod size (prover.rs:521-523, :552).
 *   trace, aux        commitments of this context with the same degree and rate; aux (NULL when there are neither lookups nor
 *                     CTLs) holds exactly the lookup columns (p2hot_stark_lookup_polys' order), then the CTL helpers, then the CTL Zs
 *   ctl_num_helpers   HOST [num_ctl_zs]: the helper columns of every Z in aux (CtlData::num_ctl_helper_polys), or NULL for what
 *                     p2hot_stark_ctl_polys produces.  0 or ceil(num_looking / chunk); 0 with more than two entries is P2HOT_EINVAL
 *   alphas            HOST [num_challenges]; the lookup challenges are num_challenges many too (StarkConfig::num_challenges)
 *   constraint_accs   NULL or [num_challenges] HOST pointers to n << qbits words, natural order: ConstraintConsumer::accumulators()
 *                     after stark.eval_packed_generic alone (the STARK's own constraints stay the caller's)
 * The consumer is a Horner in alpha (constraint_consumer.rs:68-74) and the STARK's constraints come first (vanishing_poly.rs), so
 * with K library terms c_0 .. c_{K-1} in the consumer's order -- per lookup and challenge the helper checks, constraint_first_row(z),
 * constraint((next_z - z)(t + x) - y); per Z the helper checks, constraint_last_row, constraint_transition in the three branches of
 * cross_table_lookup.rs:604-627 --
 *   value_a(x) = (constraint_accs[a][i] alpha_a^K + sum_t c_t alpha_a^(K-1-t)) / Z_H(x)
 * with z_last = x - w_n^-1, L_first(x) = Z_H(x) / (n (x - 1)), L_last(x) = Z_H(x) / (n (w_n x - 1)) (the values of the selector
 * LDEs of prover.rs:526-529).  values_out / chunks_out as in p2hot_quotient_polys (coset_ifft, trim to qdf n, chunks of n;
 * "Quotient has failed" is P2HOT_EINVAL).  constraint_degree 0 is taken as qdf = 1 (the subtraction saturates, as the chunk
 * size does; Stark::quotient_degree_factor answers 0 there and the reference computes no quotient, prover.rs:508-510), so the three
 * entry points accept the same degrees.  P2HOT_EINVAL besides the common cases: qbits > rate_bits, an aux
 * whose column count is not exactly what the descriptors imply, commitments of another context, degree or rate. */
int p2hot_stark_quotient_polys(p2hot_ctx *ctx, const p2hot_batch *trace, const p2hot_batch *aux, const p2hot_stark_tables *tables,
                               const p2hot_stark_lookup *lookups, unsigned num_lookups, const uint64_t *lookup_challenges,
                               const p2hot_stark_ctl_z *ctl_zs, unsigned num_ctl_zs, const unsigned *ctl_num_helpers,
                               unsigned constraint_degree, const uint64_t *alphas, unsigned num_challenges,
                               const uint64_t *const *constraint_accs, uint64_t *values_out, p2hot_cols **chunks_out);

/* ---------------------------------------------------------------- starky: the STARK's own constraints as a constraint program
 * Stark::eval_packed_generic (starky/src/stark.rs) is user code; here it arrives as data: a straight-line program over the
 * evaluation frame, flat HOST arrays the library uploads per call, interpreted at every point of the quotient coset (csrc/air.hpp).
 * An operand (a, b) carries its kind in the top 3 bits and an index in the low 29:
 *   P2HOT_AIR_LOCAL   trace column of the local row, get_lde_values(i, step)
 *   P2HOT_AIR_NEXT    trace column of the row at (i + 2^qbits) mod size (prover.rs:552, :568-572)
 *   P2HOT_AIR_PUBLIC  index into the call's public_inputs
 *   P2HOT_AIR_CONST   index into `constants` (any 64-bit word, reduced as p2hot_stark_term.coeff is)
 *   P2HOT_AIR_TEMP    slot < num_temps
 * Ops: ADD / SUB / MUL  temp[dst] = a op b;  CONSTRAINT, CONSTRAINT_TRANSITION, CONSTRAINT_FIRST_ROW, CONSTRAINT_LAST_ROW consume
 * `a` (dst and b are ignored): the four methods of ConstraintConsumer (constraint_consumer.rs:62-85), in program order,
 * acc_j = acc_j alpha_j + c, with c first multiplied by z_last = x - w_n^-1 / L_first(x) / L_last(x) in the three filtered ones.
 * Checked before anything is enqueued.  P2HOT_EINVAL: an unknown operand kind; a LOCAL / NEXT column beyond the trace's width; a
 * public, constant, temp or dst index beyond its count; a temp read before any instruction wrote it; null arrays with a nonzero
 * count; num_publics > 0 with null public_inputs; a constraint whose degree exceeds quotient_degree_factor + 1, the degree counted
 * in units of the trace's (LOCAL, NEXT 1; PUBLIC, CONST 0; ADD, SUB the larger; MUL the sum; the first-row and last-row filters
 * add 1, z_last does not).  P2HOT_EUNSUPPORTED: an unknown op; num_temps above p2hot_air_max_temps().  A program of num_insns == 0
 * is valid: no constraints. */
#define P2HOT_AIR_LOCAL 0u
#define P2HOT_AIR_NEXT 1u
#define P2HOT_AIR_PUBLIC 2u
#define P2HOT_AIR_CONST 3u
#define P2HOT_AIR_TEMP 4u
#define P2HOT_AIR_OPERAND(kind, index) (((uint32_t)(kind) << 29) | (uint32_t)(index))
#define P2HOT_AIR_ADD 0u
#define P2HOT_AIR_SUB 1u
#define P2HOT_AIR_MUL 2u
#define P2HOT_AIR_CONSTRAINT 3u
#define P2HOT_AIR_CONSTRAINT_TRANSITION 4u
#define P2HOT_AIR_CONSTRAINT_FIRST_ROW 5u
#define P2HOT_AIR_CONSTRAINT_LAST_ROW 6u
typedef struct p2hot_air_insn { uint32_t op, dst, a, b; } p2hot_air_insn;
typedef struct p2hot_air_program { const p2hot_air_insn *insns; const uint64_t *constants;
                                   uint32_t num_insns, num_constants, num_temps, num_publics; } p2hot_air_program;
/* the most temp slots a program may use: the interpreter keeps them in LDS, 8 bytes per slot and lane, 64 KiB per workgroup of 256 */
unsigned p2hot_air_max_temps(void);
/* ConstraintConsumer::accumulators() after Stark::eval_packed_generic alone, at every point of the quotient coset:
 * accs_out HOST [num_challenges][n << qbits], natural order -- exactly what p2hot_stark_quotient_polys takes as constraint_accs.
 * trace, constraint_degree, alphas and num_challenges as there (the same degrees, qbits <= rate_bits, no KeccakHash commitment). */
int p2hot_stark_constraint_accs(p2hot_ctx *ctx, const p2hot_batch *trace, const p2hot_air_program *program,
                                const uint64_t *public_inputs, unsigned constraint_degree, const uint64_t *alphas,
                                unsigned num_challenges, uint64_t *accs_out);
/* p2hot_stark_quotient_polys with the STARK's constraints as a program instead of host accumulators: the interpreter writes the
 * accumulators into the device buffer the lookup / CTL kernel reads, so they never cross to the host.  Every rule of
 * p2hot_stark_quotient_polys holds; an empty program is its constraint_accs = NULL. */
int p2hot_stark_quotient_polys_air(p2hot_ctx *ctx, const p2hot_batch *trace, const p2hot_batch *aux, const p2hot_stark_tables *tables,
                                   const p2hot_stark_lookup *lookups, unsigned num_lookups, const uint64_t *lookup_challenges,
                                   const p2hot_stark_ctl_z *ctl_zs, unsigned num_ctl_zs, const unsigned *ctl_num_helpers,
                                   unsigned constraint_degree, const uint64_t *alphas, unsigned num_challenges,
                                   const p2hot_air_program *program, const uint64_t *public_inputs,
                                   uint64_t *values_out, p2hot_cols **chunks_out);

/* ---------------------------------------------------------------- gate programs: the constraints of user-defined gates (D = 2)
 * A gate the table of P2HOT_GATE_* does not hold arrives as data: its eval_unfiltered_base_one as a p2hot_air_program (the same
 * p2hot_air_insn, the same operand packing) read with the GATE's frame and interpreted at every point of the quotient coset
 * (csrc/gate_program.hpp):
 *   P2HOT_AIR_LOCAL       wire column c of the row (vars.local_wires[c])
 *   P2HOT_AIR_GATE_CONST  the gate's own local_constants[c]: constants column num_selectors + num_lookup_selectors + c (gate.rs:179)
 *   P2HOT_AIR_PUBLIC      public_inputs_hash[i] of the gate set, i < num_publics <= 4
 *   P2HOT_AIR_CONST, P2HOT_AIR_TEMP  as in a constraint program;  P2HOT_AIR_NEXT is not valid here
 * An extension-algebra gate is written over pairs of base wires with W = 7.  Ops: ADD, SUB, MUL and CONSTRAINT.  The j-th CONSTRAINT
 * of a program, in program order, is constraint j of that gate -- every gate's constraints start at index 0
 * (vanishing_poly.rs:722-725) -- and is weighted by alpha^j (reduce_with_powers, not the STARK consumer's Horner form):
 *   gate_sums[a][i] += filter_g(x_i) sum_j alpha_a^j c_{g,j}(x_i)
 * with row, selector_index and [group_first, group_end) as in p2hot_gate.  Kind 5 stays P2HOT_EINVAL in a STARK's program.
 * The three entry points below are p2hot_gate_sums, p2hot_quotient_polys_gates and p2hot_quotient_polys_lookup_gates argument for
 * argument plus the programs; `gates` still supplies num_selectors, num_lookup_selectors, public_inputs_hash and the gates the
 * library knows (it may hold none), the host gate_sums residual is still added on top, and num_programs == 0 is exactly the
 * entry point without programs.  Launch order: the gate kernels, the program kernel (ONE launch for all programs of the call), the
 * lookup kernel, the permutation kernel.  Hashers as in the entry points without programs.
 * Checked before anything is enqueued, the message names the program and the instruction, *chunks_out is NULL on failure.
 * P2HOT_EINVAL: programs null with num_programs > 0; a program array null with a nonzero count; row outside its group; a group of
 * more than 256 gates; selector_index >= num_selectors; a wire index beyond the wires commitment; a gate constant that reaches
 * sigmas_first_col; a NEXT operand or an unknown operand kind; num_publics > 4; a public, constant, temp or dst index beyond its
 * count; a temp read before any instruction wrote it; a row that appears twice among the programs or also as a descriptor of the
 * gate set (it would be summed twice); a constraint whose degree -- LOCAL, GATE_CONST 1; PUBLIC, CONST 0; ADD, SUB the larger;
 * MUL the sum -- plus the filter's (group_end - group_first - 1, and 1 more when num_selectors > 1: gate.rs:326-333) exceeds
 * quotient_degree_factor + 1, the max_degree of gates/selectors.rs:101-160.  P2HOT_EUNSUPPORTED: an op outside the four (the
 * three filtered consumer ops among them); num_temps above p2hot_air_max_temps().  A program of num_insns == 0 is valid: a gate
 * without constraints. */
#define P2HOT_AIR_GATE_CONST 5u
typedef struct p2hot_gate_program { uint32_t row, selector_index, group_first, group_end;   /* as in p2hot_gate */
                                    p2hot_air_program program; } p2hot_gate_program;
int p2hot_gate_sums_programs(p2hot_ctx *ctx, const p2hot_batch *wires, const p2hot_batch *constants_sigmas, size_t sigmas_first_col,
                             const p2hot_gate_set *gates, unsigned quotient_degree_factor, const uint64_t *alphas, unsigned num_challenges,
                             uint64_t *out_host, const p2hot_gate_program *programs, unsigned num_programs);
int p2hot_quotient_polys_gate_programs(p2hot_ctx *ctx, const p2hot_batch *wires, const p2hot_batch *constants_sigmas, size_t sigmas_first_col,
                                       const p2hot_batch *zs_partial_products, const uint64_t *k_is, unsigned num_routed,
                                       unsigned quotient_degree_factor, const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas,
                                       unsigned num_challenges, const uint64_t *const *gate_sums, const p2hot_gate_set *gates,
                                       uint64_t *values_out, p2hot_cols **chunks_out, const p2hot_gate_program *programs,
                                       unsigned num_programs);
int p2hot_quotient_polys_lookup_gate_programs(p2hot_ctx *ctx, const p2hot_batch *wires, const p2hot_batch *constants_sigmas,
                                              size_t sigmas_first_col, const p2hot_batch *zs_partial_products_lookups, const uint64_t *k_is,
                                              unsigned num_routed, unsigned quotient_degree_factor, const uint64_t *betas,
                                              const uint64_t *gammas, const uint64_t *alphas, unsigned num_challenges,
                                              const uint64_t *const *gate_sums, unsigned num_lu_slots, unsigned num_lut_slots,
                                              unsigned num_luts, size_t lookup_selectors_first_col, const uint64_t *deltas,
                                              const uint64_t *lut_re_poly_evals, const p2hot_gate_set *gates, uint64_t *values_out,
                                              p2hot_cols **chunks_out, const p2hot_gate_program *programs, unsigned num_programs);

/* ================================================================ batch FRI: polynomials of several degrees, one tree, one proof
 * plonky2/src/batch_fri/{oracle,prover}.rs over hash/batch_merkle_tree.rs.  Poseidon configuration, one GPU, blinding = false: a
 * Keccak challenger or Keccak hasher bits are P2HOT_EUNSUPPORTED ("batch FRI is Poseidon-only").
 *
 * The tree (BatchMerkleTree::new, hash/batch_merkle_tree.rs:35-130).  Group j is a matrix of 2^h_j rows, h_0 > h_1 > ... (at most 8
 * groups here, more is P2HOT_EUNSUPPORTED).  Segment 0 is the Merkle forest of group 0 capped at the layer of 2^h_1 nodes; the leaf
 * i of segment j > 0 is that layer's digest i followed by row i of group j (4 + W_j words, hash_or_noop), capped at h_{j+1}; the
 * last segment is capped at cap_height <= h_last.  `digests` is the segments' digest arrays back to back, each in the MerkleTree
 * layout (merkle_tree.rs:50-57) of its own (2^h_j leaves, cap) pair: p2hot_num_digests(h_0, cap_height) digests in all.
 *   d_groups     HOST table of n_groups DEVICE pointers: group j column-major, element (row, c) at d_groups[j][c * strides[j] + row]
 *   strides, widths, log_heights  HOST [n_groups]; strides[j] >= 2^log_heights[j]
 *   d_digests    DEVICE [p2hot_num_digests(log_heights[0], cap_height)][4], d_cap DEVICE [2^cap_height][4] */
int p2hot_batch_merkle_dev(p2hot_ctx *ctx, const uint64_t *const *d_groups, const size_t *strides, const size_t *widths,
                           const unsigned *log_heights, size_t n_groups, unsigned cap_height, uint64_t *d_digests, uint64_t *d_cap);
/* BatchMerkleTree::values (batch_merkle_tree.rs:155-164) flattened, for m DEVICE leaf indices of the tallest group: row
 * idx >> (h_0 - h_j) of every group, d_out [m][sum_j W_j].  An index >= 2^h_0: see p2hot_gather_rows_dev. */
int p2hot_batch_merkle_rows_dev(p2hot_ctx *ctx, const uint64_t *const *d_groups, const size_t *strides, const size_t *widths,
                                const unsigned *log_heights, size_t n_groups, const uint64_t *d_idx, size_t m, uint64_t *d_out);
/* BatchMerkleTree::open_batch (batch_merkle_tree.rs:133-153): the merkle_tree_prove paths of the segments, concatenated:
 * d_out [m][log_heights[0] - cap_height][4].  An index >= 2^h_0: see p2hot_merkle_paths_dev. */
int p2hot_batch_merkle_paths_dev(p2hot_ctx *ctx, const uint64_t *d_digests, const unsigned *log_heights, size_t n_groups,
                                 unsigned cap_height, const uint64_t *d_idx, size_t m, uint64_t *d_out);
/* batch_fri_committed_trees (batch_fri/prover.rs:88-147): the commit phase over n_instances final polynomials of strictly decreasing
 * degree.  d_coeffs_planar: HOST table of DEVICE pointers, instance j as planes [2][2^log_n[j]] (the nonzero coefficients; the
 * reference passes instance 0 as padded coefficients and every instance as LDE values on g * H).  After round r's fold the
 * instance whose length equals the folded length joins: final_values = final_values * beta_r + values_j (:124-135) -- computed here
 * on the coefficients, s_k = beta_r f_k + p_k (g / shift')^k with shift' the coset shift after the fold, which is what the
 * reference's coset_fft, pointwise sum and coset_ifft on shift' * H yield.  Every instance must join after some round (the
 * reference's assert, :138), else P2HOT_EINVAL.  The remaining arguments and outputs are p2hot_fri_commit_dev's (with log_n[0] for
 * log_n); the Option arguments do not exist on this path. */
int p2hot_batch_fri_commit_dev(p2hot_ctx *ctx, const uint64_t *const *d_coeffs_planar, const unsigned *log_n, size_t n_instances,
                               unsigned rate_bits, unsigned cap_height, const unsigned *arity_bits, unsigned n_rounds,
                               p2hot_challenger *challenger, uint64_t *d_leaves_out, uint64_t *digests_out, int digests_on_device,
                               uint64_t *caps_out, uint64_t *betas_out, uint64_t *final_out);

/* A device-resident BatchFriOracle (batch_fri/oracle.rs:29-37): `polynomials`, one LDE matrix per group of equal degree, the
 * batch tree's digests and cap.  HOST pointers; these calls join the busy guard (see the prover session section):
 * p2hot_batch_oracle_commit / _coeffs / _rows / _paths / _digests and p2hot_batch_prove_openings.  p2hot_batch_oracle_free follows
 * the rules of p2hot_batch_free. */
typedef struct p2hot_batch_oracle p2hot_batch_oracle;
/* BatchFriOracle::from_values (is_values != 0, oracle.rs:44-66) / from_coeffs (:69-125), blinding = false.
 *   cols        W host pointers, polynomial c has 2^log_n[c] words; log_n non-increasing (the reference's assert, :81), consecutive
 *               polynomials of equal degree form a group
 *   coeffs_out  NULL or a TABLE of W host pointers (as P2HOT_COEFFS_PER_COLUMN): polynomial c's coefficients go to table[c]
 *   digests_out [p2hot_num_digests(log_n[0] + rate_bits, cap_height)][4], cap_out [2^cap_height][4]: caller-allocated or NULL
 *   flags       0 (hasher bits other than 0: P2HOT_EUNSUPPORTED; anything else: P2HOT_EINVAL)
 * P2HOT_EINVAL: W = 0, degrees out of order, cap_height above the smallest LDE height log_n[W-1] + rate_bits. */
int p2hot_batch_oracle_commit(p2hot_ctx *ctx, const uint64_t *const *cols, const unsigned *log_n, size_t W, unsigned rate_bits,
                              unsigned cap_height, int is_values, unsigned flags, uint64_t *coeffs_out, uint64_t *digests_out,
                              uint64_t *cap_out, p2hot_batch_oracle **handle_out);
size_t p2hot_batch_oracle_num_groups(const p2hot_batch_oracle *oracle);
/* width (polynomials) and degree log of group j */
int p2hot_batch_oracle_group_info(const p2hot_batch_oracle *oracle, size_t group, size_t *width_out, unsigned *degree_log_out);
/* `polynomials[first .. first + count)` in commit order, canonical, back to back (each with its own length) */
int p2hot_batch_oracle_coeffs(p2hot_batch_oracle *oracle, size_t first, size_t count, uint64_t *out);
/* BatchMerkleTree::values flattened for m leaf indices of the tallest group: out [m][sum_j W_j] */
int p2hot_batch_oracle_rows(p2hot_batch_oracle *oracle, const uint64_t *row_idx, size_t m, uint64_t *out);
/* BatchMerkleTree::open_batch: out [m][log_n[0] + rate_bits - cap_height][4] */
int p2hot_batch_oracle_paths(p2hot_batch_oracle *oracle, const uint64_t *leaf_idx, size_t m, uint64_t *out);
/* batch_merkle_tree.digests: out [p2hot_num_digests(log_n[0] + rate_bits, cap_height)][4] */
int p2hot_batch_oracle_digests(p2hot_batch_oracle *oracle, uint64_t *out);
void p2hot_batch_oracle_free(p2hot_batch_oracle *oracle);
/* FriInstanceInfo::batches (fri/structure.rs) of one instance = one degree; poly_index counts the oracle's polynomials in commit order */
typedef struct p2hot_fri_instance { const p2hot_fri_batch_info *batches; size_t n_batches; } p2hot_fri_instance;
/* the p2hot_fri_proof layout of p2hot_batch_prove_openings: initial_leaves [Q][sum_o sum_j W_{o,j}], initial_paths
 * [Q][n_oracles][h_0 - cap_height][4], the rest as p2hot_fri_proof_sizes with the first oracle's largest degree.  No context, so no
 * error text; the sizes hold only for oracles p2hot_batch_prove_openings accepts together (one context, rate, cap height and tallest
 * height): it is that call which checks them. */
int p2hot_batch_fri_proof_sizes(const p2hot_batch_oracle *const *oracles, size_t n_oracles, const p2hot_fri_params *params,
                                p2hot_fri_proof_layout *out);
/* BatchFriOracle::prove_openings (batch_fri/oracle.rs:128-192) + batch_fri_proof (batch_fri/prover.rs:25-86): alpha once, one
 * final_poly per instance (the prelude of p2hot_prove_openings per degree), the batch commit phase, the grind (smallest witness),
 * the query rounds over the batch trees (:175-217); one synchronisation, the challenges stay on the device.
 * Validated before anything is enqueued (the context stays usable).  P2HOT_EINVAL: n_instances = 0; degree_bits not strictly
 * decreasing; an oracle of another context, or whose tallest group is not 2^(degree_bits[0] + rate_bits) rows, or committed with
 * another rate / cap height; a polynomial opened by instance i whose degree is not 2^degree_bits[i]; an instance whose length is not
 * reached exactly after some round; a round tree smaller than the cap; non-zero max_num_query_steps or final_poly_coeff_len.
 * P2HOT_EUNSUPPORTED: a Keccak challenger. */
int p2hot_batch_prove_openings(p2hot_ctx *ctx, const unsigned *degree_bits, const p2hot_fri_instance *instances, size_t n_instances,
                               const p2hot_batch_oracle *const *oracles, size_t n_oracles, p2hot_challenger *challenger,
                               const p2hot_fri_params *params, p2hot_fri_proof *proof);

/* ================================================================ multi-GPU: the coset-sharded commit
 * The rate-1/B LDE is B independent coset transforms and coset j is the contiguous row block bitrev(j) of the
 * committed order, so rank r of G owns rows [r*N/G, (r+1)*N/G) = whole cosets = whole cap subtrees: it runs the LDE,
 * the leaf sponge and the Merkle levels of its rows with no data-path exchange.  Exchanges: the coefficients after the
 * column-sharded iNTT (W*n*8 bytes, pipelined in column chunks beside the transforms), the 2^cap_height cap entries,
 * and -- on request -- the digest slices.  G <= 2^cap_height, G a power of two.  G > 2^rate_bits (starky's rate-1/2 traces on 4 or
 * 8 GPUs): the cosets are split into sub-cosets of H_n -- rank r folds every polynomial mod x^n' - c_r (n' = N/G rows, c_r = the
 * n'-th power of its block's coset shift) and runs the same LDE at (log n', log(N/n')); same exchange, same results.
 * Two ways to run it:
 *   one process per GPU   p2hot_comm_create_rccl (RCCL over xGMI; the launcher distributes the unique id) or
 *                         p2hot_comm_create_callback (the host application's own all-gather), then p2hot_commit_sharded_dev
 *   one process, N GPUs   p2hot_group_create + p2hot_group_commit: host pointers in, like p2hot_commit -- a patched
 *                         plonky2 gets every GPU of the node from its main thread
 * RCCL is bound at run time (dlopen), libp2hot.so has no link-time dependency on it. */
#define P2HOT_UNIQUE_ID_BYTES 128 /* NCCL_UNIQUE_ID_BYTES, rccl.h:40 */
typedef struct p2hot_comm p2hot_comm;
typedef struct p2hot_group p2hot_group;
typedef struct p2hot_sharded_batch p2hot_sharded_batch;
/* caller-supplied transport: rank r's slice is `bytes` bytes at d_base + offsets[r] (valid on rank r); on return every
 * slice must be complete on this rank.  Called on the host with the context's stream idle; return 0 on success. */
typedef int (*p2hot_allgather_fn)(void *user, void *d_base, const size_t *offsets, int world, size_t bytes, void *hip_stream);
int p2hot_comm_unique_id(uint8_t out[P2HOT_UNIQUE_ID_BYTES]);               /* ncclGetUniqueId on one rank */
int p2hot_comm_create_rccl(p2hot_ctx *ctx, int rank, int world, const uint8_t id[P2HOT_UNIQUE_ID_BYTES], p2hot_comm **out);
int p2hot_comm_create_callback(p2hot_ctx *ctx, int rank, int world, p2hot_allgather_fn fn, void *user, p2hot_comm **out);
void p2hot_comm_destroy(p2hot_comm *comm);
int p2hot_comm_rank(const p2hot_comm *comm);
int p2hot_comm_world(const p2hot_comm *comm);
/* preflight (collective: every rank calls it): a `bytes`-sized pattern slice per rank is all-gathered the way the commit
 * exchanges coefficients and caps, and every rank checks every slice; P2HOT_ECOMM with a named cause on failure */
int p2hot_comm_selftest(p2hot_comm *comm, size_t bytes);
/* How equal, contiguous slices (whole-rank coefficient slices, cap, digest slices; the pipelined column chunks through a
 * chunk-major staging block) travel on an RCCL transport: 0 = one grouped ncclBroadcast per slice, 1 = ncclAllGather.  On an
 * RCCL communicator p2hot_comm_selftest checks and times both and keeps the faster (rank 0's verdict, broadcast to all);
 * p2hot_group_create does the same over its ranks; P2HOT_EXCHANGE=broadcast|allgather pins one.  -1 for a null handle. */
int p2hot_comm_exchange_mode(const p2hot_comm *comm);
/* Which RCCL this process is bound to: the library file (dladdr of ncclGetUniqueId) into path_out (NUL-terminated, truncated to
 * path_cap) and ncclGetVersion's code (e.g. 22203) into version_out; either may be NULL.  The library prefers the copy the
 * process already loaded (PyTorch's, under torch.distributed.run) and falls back to /opt/rocm/lib/librccl.so.1 by path (a patched
 * plonky2, no torch): two deployment modes, two RCCL builds -- a run reports which one it used.  P2HOT_ECOMM if none binds. */
int p2hot_rccl_info(char *path_out, size_t path_cap, int *version_out);
/* columns [first, first + count) of W are the ones rank `rank` of `world` transforms in the iNTT stage */
int p2hot_shard_columns(size_t W, int world, int rank, size_t *first, size_t *count);
/* from_values / from_coeffs (fri/oracle.rs:57-112) of this rank's share, DEVICE pointers, asynchronous:
 *   d_cols_local  [count][n] this rank's columns (p2hot_shard_columns), stride col_stride
 *   d_coeffs_all  [world * ceil(W/world)][n] out: row c = polynomial c for c < W (`polynomials`, complete on every rank)
 *   d_lde         [W][N/world] out: this rank's rows of the LDE matrix, column-major, stride lde_stride
 *   d_leaves      [N/world][W] out or NULL
 *   d_digests, d_cap: FULL-tree arrays; this rank's digest slice [rank * nd/world, +nd/world) and the whole cap are
 *                 valid on return, the other digest slices only with gather_digests != 0 (a Merkle path below the
 *                 cap never leaves the cap subtree of its leaf: the owner of a row can always serve its path)
 *   pipeline_chunks: column chunks of the coefficient exchange (0 / 1 = one blocking exchange; 8 is a good default) */
int p2hot_commit_sharded_dev(p2hot_ctx *ctx, p2hot_comm *comm, const uint64_t *d_cols_local, size_t col_stride, size_t W,
                             unsigned log_n, unsigned rate_bits, unsigned cap_height, int is_values, int gather_digests,
                             unsigned pipeline_chunks, uint64_t *d_coeffs_all, uint64_t *d_lde, size_t lde_stride,
                             uint64_t *d_leaves, uint64_t *d_digests, uint64_t *d_cap);
/* one process, n_gpus devices (devices == NULL: 0 .. n_gpus-1), one context + stream per device.  Distinct devices use
 * RCCL (ncclCommInitAll); a repeated device id (one-GPU test boxes) or P2HOT_GROUP_PEER_COPY=1 uses peer copies. */
int p2hot_group_create(int n_gpus, const int *devices, p2hot_group **out);
void p2hot_group_destroy(p2hot_group *group);
int p2hot_group_size(const p2hot_group *group);
p2hot_ctx *p2hot_group_ctx(p2hot_group *group, int i);
int p2hot_group_uses_rccl(const p2hot_group *group);
int p2hot_group_exchange_mode(const p2hot_group *group); /* see p2hot_comm_exchange_mode */
const char *p2hot_group_last_error(const p2hot_group *group);
/* from_values / from_coeffs over every GPU of the group, HOST pointers (the multi-GPU p2hot_commit): each GPU is sent
 * only the columns it transforms; coeffs_out / leaves_out / digests_out / cap_out (any may be NULL) are assembled from
 * the owning ranks.  handle_out: the sharded batch for p2hot_sharded_batch_open. */
int p2hot_group_commit(p2hot_group *group, const uint64_t *const *cols, size_t W, unsigned log_n, unsigned rate_bits,
                       unsigned cap_height, int is_values, int shard_mode, unsigned pipeline_chunks, uint64_t *coeffs_out,
                       uint64_t *leaves_out, uint64_t *digests_out, uint64_t *cap_out, p2hot_sharded_batch **handle_out);
/* shard_mode: P2HOT_SHARD_COSETS (default design, above) or P2HOT_SHARD_COLUMNS -- the fallback of SURVEY 8e's last row:
 * each rank runs the iNTT and the WHOLE LDE of its ceil(W/G) columns, then the LDE matrix is re-partitioned to row blocks
 * by an all-to-all of strided peer copies (the leaf sponge chains across the columns of a row) before hashing.  It moves
 * W*N*8 bytes instead of W*n*8 (2^rate_bits times more); kept as a second, independently derived partition (the coset mode
 * serves G > 2^rate_bits by sub-cosets).  Same results bit for bit. */
#define P2HOT_SHARD_COSETS 0
#define P2HOT_SHARD_COLUMNS 1
/* MerkleTree::get + merkle_tree_prove (merkle_tree.rs:227, :151-190) for m leaves, each answered by the rank that owns
 * the row: rows_out [m][W], paths_out [m][log2(N) - cap_height][4]; either may be NULL */
int p2hot_sharded_batch_open(p2hot_sharded_batch *batch, const uint64_t *leaf_idx, size_t m, uint64_t *rows_out, uint64_t *paths_out);
void p2hot_sharded_batch_free(p2hot_sharded_batch *batch);
/* OpeningSet::new, p2hot_fri_proof_sizes and PolynomialBatch::prove_openings + fri_proof (see the single-GPU entry points
 * above) over sharded oracles of one group, coset mode only (every rank then holds all coefficients): rank 0 runs what
 * needs the polynomials -- the evaluations, final_poly, the FRI commit phase (tiny after round 0), the grind --
 * and the rows and Merkle paths of the initial trees come from the ranks that own them.  `challenger` belongs to
 * p2hot_group_ctx(group, 0).  Same proof, bit for bit, as the single-GPU path on the same polynomials. */
int p2hot_group_eval_openings(p2hot_group *group, const p2hot_sharded_batch *const *oracles, size_t n_oracles, const uint64_t *points,
                              size_t n_points, uint64_t *out);
int p2hot_group_fri_proof_sizes(const p2hot_sharded_batch *const *oracles, size_t n_oracles, const p2hot_fri_params *params,
                                p2hot_fri_proof_layout *out);
int p2hot_group_prove_openings(p2hot_group *group, const p2hot_fri_batch_info *batches, size_t n_batches,
                               const p2hot_sharded_batch *const *oracles, size_t n_oracles, p2hot_challenger *challenger,
                               const p2hot_fri_params *params, p2hot_fri_proof *proof);

#ifdef __cplusplus
}
#endif
#endif
