// host_prover.hpp -- the HOST-POINTER layer of libp2hot: what a patched plonky2 crate calls from the prover's main thread
// with ordinary Vec<F> buffers (include/p2hot.h, "prover session" section).  Included at the end of p2hot.hip (one TU): the
// commitments, the OpeningSet and the opening proof here, the middle of a proof (permutation argument, lookups, quotient) in host_plonk.hpp.
//
// Reference call sites this layer stands behind:
//   PolynomialBatch::from_values / from_coeffs   plonky2/src/fri/oracle.rs:57-112      p2hot_commit, p2hot_commit_cols
//   MerkleTree::get / ::prove                      hash/merkle_tree.rs:227, :231-237     p2hot_batch_rows, p2hot_batch_paths
//   OpeningSet::new                                plonk/proof.rs:314-327                p2hot_eval_openings
//   PolynomialBatch::prove_openings + fri_proof    fri/oracle.rs:176-237, fri/prover.rs:24-82, :204-258   p2hot_prove_openings
// Everything between the calls stays on the GPU behind opaque handles (p2hot_batch, p2hot_cols, p2hot_challenger).
#pragma once

#include <atomic>
#include <functional>
#include <thread>

// one call at a time per context: a second thread entering gets P2HOT_EBUSY instead of a data race on the scratch blocks
struct CallGuard {
    p2hot_ctx *ctx;
    bool ok;
    explicit CallGuard(p2hot_ctx *c) : ctx(c), ok(false) {
        if (ctx) ok = !ctx->busy.exchange(true, std::memory_order_acquire);
        if (ok) ctx->in_host_call = true;
    }
    ~CallGuard() {
        if (!ok) return;
        ctx->in_host_call = false;
        ctx->deferred.clear();  // a call that failed before its synchronisation delivers nothing
        ctx->pinned_used = 0;
        ctx->busy.store(false, std::memory_order_release);
    }
};
#define P2_ENTER(ctx)                                                                                                  \
    CallGuard guard_(ctx);                                                                                             \
    DeviceGuard dev_guard_(ctx);                                                                                       \
    if (!(ctx)) return P2HOT_EINVAL;                                                                                   \
    if (!guard_.ok) return P2HOT_EBUSY /* the context's error text belongs to the call that is running */

static int sync_checked(p2hot_ctx *ctx, int rc, const char *what) {
    hipError_t e = stream_sync(ctx);
    if (rc == P2HOT_OK && e != hipSuccess) P2_FAIL(ctx, P2HOT_EHIP, "%s: %s", what, hipGetErrorString(e));
    return rc;
}

// ------------------------------------------------------------------ device-resident column sets
extern "C" int p2hot_cols_upload(p2hot_ctx *ctx, const uint64_t *const *cols, size_t W, unsigned log_n, p2hot_cols **out) {
    P2_ENTER(ctx);
    if (!out) P2_FAIL(ctx, P2HOT_EINVAL, "cols_upload: null output");
    *out = nullptr;
    P2_TRY(check_log(ctx, log_n, "cols_upload"));
    if (W > 0 && !cols) P2_FAIL(ctx, P2HOT_EINVAL, "cols_upload: null column table");
    const size_t n = (size_t)1 << log_n;
    PoolBuf d(ctx);
    P2_TRY(pool_alloc(ctx, (W ? W : 1) * n * 8, &d.p));
    for (size_t c = 0; c < W; ++c)
        if (!cols[c]) P2_FAIL(ctx, P2HOT_EINVAL, "cols_upload: column %zu is null", c);
    P2_TRY(h2d_columns(ctx, d.u(), cols, W, n * 8, 0, W * n * 8, ctx->stream));
    P2_TRY(sync_checked(ctx, P2HOT_OK, "cols_upload"));
    *out = new p2hot_cols{ctx, d.u(), W, log_n, true};
    d.p = nullptr;
    return P2HOT_OK;
}

extern "C" int p2hot_cols_download(p2hot_cols *c, size_t first, size_t count, uint64_t *out) {
    if (!c) return P2HOT_EINVAL;
    p2hot_ctx *ctx = c->ctx;
    P2_ENTER(ctx);
    if (first > c->W || count > c->W - first) P2_FAIL(ctx, P2HOT_EINVAL, "cols_download: columns [%zu,+%zu) of %zu", first, count, c->W);
    if (count == 0) return P2HOT_OK;
    if (!out) P2_FAIL(ctx, P2HOT_EINVAL, "cols_download: null output");
    const size_t n = (size_t)1 << c->log_n;
    P2_HIP(ctx, hipMemcpyAsync(out, c->d + first * n, count * n * 8, hipMemcpyDeviceToHost, ctx->stream));
    return sync_checked(ctx, P2HOT_OK, "cols_download");
}

extern "C" size_t p2hot_cols_width(const p2hot_cols *c) { return c ? c->W : 0; }
extern "C" unsigned p2hot_cols_degree_log(const p2hot_cols *c) { return c ? c->log_n : 0; }

extern "C" void p2hot_cols_free(p2hot_cols *c) {
    if (!c) return;
    if (c->owned) {
        (void)hipStreamSynchronize(c->ctx->stream);
        pool_release(c->ctx, c->d);
    }
    delete c;
}

// ------------------------------------------------------------------ from_values / from_coeffs
static p2hot_batch *make_batch(p2hot_ctx *ctx, PoolBuf &lde, PoolBuf &dig, PoolBuf &coef, PoolBuf *vals, size_t W, unsigned log_n,
                               unsigned rate_bits, unsigned cap_height, size_t S = 0) {
    p2hot_batch *b = new p2hot_batch{ctx, lde.u(), W, ((size_t)1 << log_n) << rate_bits, dig.u(), log_n + rate_bits, cap_height};
    b->S = S;
    b->d_coef = coef.u();
    b->d_vals = vals ? vals->u() : nullptr;
    b->log_n = log_n;
    b->rate_bits = rate_bits;
    lde.p = dig.p = coef.p = nullptr;  // ownership moves to the handle (still live blocks of the context's cache)
    if (vals) vals->p = nullptr;
    return b;
}

// from_values / from_coeffs with host pointers; S salt columns (blinding = true: oracle.rs:123-137) or none
static int commit_host(p2hot_ctx *ctx, const uint64_t *const *cols, size_t W, unsigned log_n, unsigned rate_bits,
                       unsigned cap_height, int is_values, unsigned flags, const uint64_t *const *salt_cols, size_t S,
                       uint64_t *coeffs_out, uint64_t *leaves_out, uint64_t *digests_out, uint64_t *cap_out,
                       p2hot_batch **handle_out) {
    P2_ENTER(ctx);
    if (handle_out) *handle_out = nullptr;
    if (S && !salt_cols) P2_FAIL(ctx, P2HOT_EINVAL, "commit: null salt column table");
    for (size_t j = 0; j < S; ++j)
        if (!salt_cols[j]) P2_FAIL(ctx, P2HOT_EINVAL, "commit: salt column %zu is null", j);
    P2_TRY(check_log(ctx, log_n + rate_bits, "commit"));
    if (W == 0) P2_FAIL(ctx, P2HOT_EINVAL, "commit: no polynomials (the reference panics on polynomials[0], fri/oracle.rs:90)");
    if (!cols) P2_FAIL(ctx, P2HOT_EINVAL, "commit: null column table");
    if (flags & ~(unsigned)(P2HOT_KEEP_VALUES | P2HOT_COEFFS_PER_COLUMN | P2HOT_LEAVES_ASYNC | P2HOT_LEAVES_NATURAL | P2HOT_HASH_MASK))
        P2_FAIL(ctx, P2HOT_EINVAL, "commit: unknown flags %#x", flags);
    const unsigned hash_n = (flags & P2HOT_HASH_MASK) >> 8;  // 0 = Poseidon, else KeccakHash<hash_n>
    if (hash_n) P2_TRY(check_hash_size(ctx, hash_n, "commit"));
    if ((flags & P2HOT_LEAVES_ASYNC) && !(leaves_out && handle_out))
        P2_FAIL(ctx, P2HOT_EINVAL, "commit: P2HOT_LEAVES_ASYNC needs leaves_out and handle_out (the handle owns the copy in flight)");
    if ((flags & P2HOT_LEAVES_NATURAL) && !leaves_out) P2_FAIL(ctx, P2HOT_EINVAL, "commit: P2HOT_LEAVES_NATURAL without leaves_out");
    const bool async_leaves = (flags & P2HOT_LEAVES_ASYNC) != 0;
    // P2HOT_COEFFS_PER_COLUMN: coeffs_out is a table of W host pointers (one Vec per polynomial on the caller's side)
    uint64_t *const *coeffs_cols = (flags & P2HOT_COEFFS_PER_COLUMN) ? reinterpret_cast<uint64_t *const *>(coeffs_out) : nullptr;
    if (coeffs_cols)
        for (size_t c = 0; c < W; ++c)
            if (!coeffs_cols[c]) P2_FAIL(ctx, P2HOT_EINVAL, "commit: coefficient destination %zu is null", c);
    const size_t n = (size_t)1 << log_n, N = n << rate_bits;
    const unsigned log_N = log_n + rate_bits;
    if (cap_height > log_N) P2_FAIL(ctx, P2HOT_EINVAL, "commit: cap_height %u > log2(N) %u (merkle_tree.rs:195-200)", cap_height, log_N);
    for (size_t c = 0; c < W; ++c)
        if (!cols[c]) P2_FAIL(ctx, P2HOT_EINVAL, "commit: column %zu is null", c);
    const size_t nd = p2hot_num_digests(log_N, cap_height), cap_words = (size_t)4 << cap_height;
    const bool keep_vals = is_values && handle_out && (flags & P2HOT_KEEP_VALUES);
    PoolBuf d_work(ctx), d_vals(ctx), d_lde(ctx), d_leaves(ctx), d_dig(ctx), d_cap(ctx);
    const size_t LW = W + S;  // leaf width
    const size_t Wn = (W ? W : 1) * n * 8, WN = (LW ? LW : 1) * N * 8;
    PoolBuf d_salt(ctx);
    P2_TRY(pool_alloc(ctx, Wn, &d_work.p));  // uploaded columns; becomes the coefficients in place
    if (keep_vals) P2_TRY(pool_alloc(ctx, Wn, &d_vals.p));
    P2_TRY(pool_alloc(ctx, WN, &d_lde.p));
    if (leaves_out) P2_TRY(pool_alloc(ctx, WN, &d_leaves.p));
    if (S) P2_TRY(pool_alloc(ctx, S * N * 8, &d_salt.p));
    P2_TRY(pool_alloc(ctx, (nd ? nd : 1) * 32, &d_dig.p));
    P2_TRY(pool_alloc(ctx, cap_words * 8, &d_cap.p));
    // The PCIe copies run on the side stream beside the compute stream.  Column blocks are uploaded, transformed (iNTT)
    // and extended (LDE) one after the other -- the upload of block b+1 overlaps the transforms of block b -- and the
    // coefficient blocks go back to the host while the leaf sponge runs.  Small batches are one block.
    const size_t kBlockCols = ctx->host_block_cols ? ctx->host_block_cols : (W >= 32 && W * n >= ((size_t)1 << 22)) ? 16 : (W ? W : 1);
    // block b = columns [blk0[b], blk0[b + 1]).  The first upload has nothing to hide behind, so when there are several blocks
    // the first one is half as wide (a multiple of the sponge rate where it can be)
    std::vector<size_t> blk0;
    {
        size_t c = 0;
        const size_t first = (!ctx->host_block_cols && kBlockCols >= 16 && W > kBlockCols) ? kBlockCols / 2 : kBlockCols;
        while (c < W) {
            blk0.push_back(c);
            c += (c == 0 ? first : kBlockCols);
        }
        blk0.push_back(W);
    }
    const size_t nb = W ? blk0.size() - 1 : 0;
    std::vector<hipEvent_t> up, done;
    hipStream_t copy_stream = ctx->stream;
    // a large leaf matrix going back to the host gets the copy stream even when the columns are one block (W < 32: the Zs and
    // quotient commitments): its copy then runs beside the sponge as well
    const bool big_leaves = ctx->host_leaves_first && leaves_out && LW && nb >= 1 && LW * N * 8 >= ((size_t)64 << 20);
    const bool two_streams = nb > 1 || big_leaves;
    if (two_streams) copy_stream = ctx->side;
    // With more than one block the leaf sponge does not wait for the last column: after each block's LDE it absorbs the
    // 8-column chunks that are complete (its state parked in a scratch block between launches), so the hashing -- three
    // quarters of the commit -- runs beside the uploads still in flight instead of behind them.
    // (not when the row-major leaf matrix goes back as well: that copy -- 9 GB at C3 -- is the long pole and can start as soon
    // as every column is extended, so the transforms run first and the whole sponge runs beside the copy instead)
    // P2HOT_LEAVES_ASYNC with several column blocks: THREE compute / copy lanes.  The transforms (upload-bound: 25 ms for 10 ms of
    // kernels at the C3 wires shape) and the transposition run on a stream of their own, so the leaf matrix exists -- and starts
    // leaving on the leaf stream -- as early as in the leaves-first order; the leaf sponge absorbs each block's columns on the
    // context's stream BESIDE them (the chunked order: the hashing, three quarters of the call, hides the uploads), so the call
    // returns as early as a call without leaves.  Neither single-stream order gives both (profiles/r05_async_ab.txt).
    // (a Keccak tree hashes after the last column instead: profiles/keccak_commit.json has what the chunked Poseidon order saves)
    const bool xsplit = !hash_n && async_leaves && ctx->host_chunked_hash && ctx->host_async_split && nb > 1 && LW > 8 && LW <= 0xFFFFFFFFull;
    const bool leaves_first = ctx->host_leaves_first && leaves_out && LW && (nb > 1 || big_leaves) && !xsplit;
    const bool early_transpose = async_leaves && LW;  // the asynchronous copy: the matrix is transposed as soon as the last column is extended
    const bool chunked = !hash_n && ctx->host_chunked_hash && nb > 1 && LW > 8 && LW <= 0xFFFFFFFFull && !leaves_first;
    PoolBuf d_state(ctx);
    ForestGeom geom{};
    unsigned hashed = 0;  // columns the sponge has absorbed (a multiple of 8 until the end)
    if (chunked) {
        P2_TRY(pool_alloc(ctx, (size_t)12 * N * 8, &d_state.p));
        P2_TRY(forest_geom(ctx, log_N, cap_height, 0, N, d_dig.u(), d_cap.u(), &geom));
    }
    // When the digests go back to the host the tail -- the last chunk(s) of the sponge and the tree levels -- runs per group of
    // cap subtrees: a group's slice of the digest array is contiguous in the reference layout, so it can travel while the next
    // groups are hashed.  (A copy into pageable memory holds the calling thread until it is done: every group's kernels are
    // enqueued first, the copies are issued after them.)
    size_t tail_groups = 1;
    if (chunked && digests_out && nd)
        while (tail_groups < 8 && tail_groups * 2 <= ((size_t)1 << cap_height) && (N / (tail_groups * 2)) >= ctx->host_tail_min_leaves)
            tail_groups *= 2;
    std::vector<hipEvent_t> tail_ev;
    [[maybe_unused]] hipEvent_t leaves_ev = nullptr;
    const unsigned leaf_rev = (flags & P2HOT_LEAVES_NATURAL) ? log_N : 0u;  // (log_N == 0: one row, nothing to reverse)
    p2hot_batch::LeafCopy *leafcopy = nullptr;  // P2HOT_LEAVES_ASYNC: handed to the batch handle at the end
    const hipStream_t main_stream = ctx->stream;
    struct StreamRestore {  // the transform lane borrows `ctx->stream` (every transform launches "on the context's stream"): given back on every path
        p2hot_ctx *c;
        hipStream_t s;
        ~StreamRestore() { c->stream = s; }
    } stream_restore{ctx, main_stream};
    std::vector<hipEvent_t> lde_ev;  // xsplit: block b is extended (transform lane -> sponge lane)
    auto absorb_upto = [&](size_t cols_done, bool may_finish) -> int {  // cols_done leaf columns of d_lde are final
        const unsigned end = (cols_done >= LW && may_finish) ? (unsigned)LW : (unsigned)((cols_done < LW ? cols_done : LW - 1) / 8 * 8);
        if (end <= hashed) return P2HOT_OK;
        P2_TRY(hash_leaves_chunks(ctx, main_stream, merkle::ColMajorReader{d_lde.u(), N}, LW, geom, N, hashed, end, d_state.u(), N));
        hashed = end;
        return P2HOT_OK;
    };
    auto issue_leaf_blocks = [&](size_t k0, size_t k1) -> int {  // blocks [k0, k1) of the asynchronous leaf copy, one event each
        const size_t bw = leafcopy->rows_per_block * LW;           // words per block
        for (size_t k = k0; k < k1; ++k) {
            P2_HIP(ctx, hipMemcpyAsync(leaves_out + k * bw, d_leaves.u() + k * bw, bw * 8, hipMemcpyDeviceToHost, ctx->leaf_stream));
            hipEvent_t e;
            P2_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventBlockingSync));
            leafcopy->ev.push_back(e);
            P2_HIP(ctx, hipEventRecord(e, ctx->leaf_stream));
        }
        return P2HOT_OK;
    };
    auto body = [&]() -> int {
        if (two_streams) {
            for (size_t b = 0; b < 2 * nb; ++b) {
                hipEvent_t e;
                P2_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
                (b < nb ? up : done).push_back(e);
            }
            // the side stream must not start before work already queued on the compute stream has finished with the blocks
            P2_HIP(ctx, hipEventRecord(ctx->join_event, ctx->stream));
            P2_HIP(ctx, hipStreamWaitEvent(ctx->side, ctx->join_event, 0));
        }
        if (xsplit) {  // the transform lane: behind whatever the context's stream already holds, then on its own
            if (!ctx->xform_stream) P2_HIP(ctx, hipStreamCreateWithFlags(&ctx->xform_stream, hipStreamNonBlocking));
            P2_HIP(ctx, hipStreamWaitEvent(ctx->xform_stream, ctx->join_event, 0));
            for (size_t b = 0; b < nb; ++b) {
                hipEvent_t e;
                P2_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
                lde_ev.push_back(e);
            }
            ctx->stream = ctx->xform_stream;  // (until the transposition below; StreamRestore covers the error paths)
        }
        for (size_t b = 0; b < nb; ++b) {
            const size_t c0 = blk0[b], cnt = blk0[b + 1] - c0;
            u64 *blk = d_work.u() + c0 * n;
            u64 *land = keep_vals ? d_vals.u() + c0 * n : blk;  // where the upload lands
            P2_TRY(h2d_columns(ctx, land, cols + c0, cnt, n * 8, c0 * n * 8, W * n * 8 + S * N * 8, copy_stream));
            if (two_streams) {
                P2_HIP(ctx, hipEventRecord(up[b], ctx->side));
                P2_HIP(ctx, hipStreamWaitEvent(ctx->stream, up[b], 0));
            }
            if (keep_vals) P2_HIP(ctx, hipMemcpyAsync(blk, land, cnt * n * 8, hipMemcpyDeviceToDevice, ctx->stream));
            if (is_values) {  // "IFFT" (oracle.rs:65-69): the block becomes its coefficients in place
                P2_TRY(ntt_natural(ctx, blk, cnt, n, log_n, true));
            } else if (coeffs_out) {
                P2HOT_LAUNCH(ntt::canon_kernel, dim3(cdiv(cnt * n, 256)), dim3(256), 0, ctx->stream, blk, cnt * n);
                P2_LAUNCH_CHECK(ctx);
            }
            if (two_streams) P2_HIP(ctx, hipEventRecord(done[b], ctx->stream));
            P2_TRY(p2hot_coset_lde_dev(ctx, blk, cnt, n, log_n, rate_bits, gl::COSET_SHIFT, 0, N, d_lde.u() + c0 * N, N));
            if (xsplit) {  // the sponge lane picks the block up when it is extended
                P2_HIP(ctx, hipEventRecord(lde_ev[b], ctx->stream));
                P2_HIP(ctx, hipStreamWaitEvent(main_stream, lde_ev[b], 0));
            }
            if (chunked) P2_TRY(absorb_upto(c0 + cnt, tail_groups == 1 && !S && !xsplit));  // (a grouped tail, and the split lanes, keep the last chunk)
        }
        if (S) {
            // the salt vectors are LDE-value columns in natural order (oracle.rs:133-137): like the LDE values they reach the
            // leaves through transpose + reverse_index_bits (:97-98), i.e. column W + j of the committed matrix is salt_j[bitrev(r)]
            // (the pinned staging block is shared with the column uploads still in flight: the salts take the slots behind them)
            P2_TRY(h2d_columns(ctx, d_salt.u(), salt_cols, S, N * 8, W * n * 8, W * n * 8 + S * N * 8, ctx->stream));
            P2_TRY(launch_bitrev(ctx, d_salt.u(), d_lde.u() + W * N, S, N, N, log_N));
        }
        if (leaves_first || early_transpose) {  // the row-major matrix before the sponge('s tail): its copy starts while the leaves are hashed
            P2_TRY(transpose_rows(ctx, d_lde.u(), N, LW, N, d_leaves.u(), leaf_rev));
            if (two_streams || async_leaves) {
                P2_HIP(ctx, hipEventCreateWithFlags(&leaves_ev, hipEventDisableTiming));
                P2_HIP(ctx, hipEventRecord(leaves_ev, ctx->stream));
            }
        }
        if (early_transpose) {
            // the matrix leaves in row blocks on a stream of its own, each block fenced by an event; this call does not wait for it.
            // The first quarter of the blocks goes now, beside the leaf sponge; the rest is queued BEHIND the digests' copy (below):
            // the 0.5 GB of digests are what this call still waits for, and they would share the link with 9 GB of leaves otherwise
            if (!ctx->leaf_stream) P2_HIP(ctx, hipStreamCreateWithFlags(&ctx->leaf_stream, hipStreamNonBlocking));
            P2_HIP(ctx, hipStreamWaitEvent(ctx->leaf_stream, leaves_ev, 0));
            leafcopy = new p2hot_batch::LeafCopy();
            leafcopy->ev.reserve(66);
            leafcopy->rows = N;
            leafcopy->aux = leaves_ev;  // the leaf stream's wait on it may not have run yet: destroyed with the copy, not with this call
            leaves_ev = nullptr;
            size_t blocks = 64;
            while (blocks > 1 && N / blocks < 1024) blocks >>= 1;  // (rows per block stays a power of two: N is one)
            leafcopy->rows_per_block = N / blocks;
            // how many blocks leave BEFORE the digests' copy is queued.  Measured at the C3 wires shape (profiles/r05_async_ab.txt): beside
            // the chunked sponge every early block costs the call ~7 ms (the copy and the sponge share the chip) and buys the last row
            // nothing -> none; in the single-stream leaves-first order a quarter of them moves the last row from 251 to 220 ms for 10 ms
            size_t early = ctx->host_async_early_blocks != (size_t)-1 ? ctx->host_async_early_blocks : (xsplit ? 0 : blocks / 4);
            if (early > blocks || !(digests_out && nd)) early = blocks;
            P2_TRY(issue_leaf_blocks(0, early));
        }
        if (xsplit) {  // the transform lane is done: the salts and the transposition were its last work; the sponge's tail waits for them
            P2_HIP(ctx, hipEventRecord(ctx->join_event, ctx->stream));
            ctx->stream = main_stream;
            P2_HIP(ctx, hipStreamWaitEvent(main_stream, ctx->join_event, 0));
        }
        if (chunked && tail_groups > 1) {
            const size_t cnt = N / tail_groups;
            for (size_t g = 0; g < tail_groups; ++g) {
                ForestGeom gg;
                P2_TRY(forest_geom(ctx, log_N, cap_height, g * cnt, cnt, d_dig.u(), d_cap.u(), &gg));
                P2_TRY(hash_leaves_chunks(ctx, ctx->stream, merkle::ColMajorReader{d_lde.u() + g * cnt, N}, LW, gg, cnt, hashed,
                                          (unsigned)LW, d_state.u() + g * cnt, N));
                P2_TRY(merkle_levels(ctx, gg, cnt));
                if (two_streams) {
                    hipEvent_t e;
                    P2_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
                    tail_ev.push_back(e);
                    P2_HIP(ctx, hipEventRecord(e, ctx->stream));
                }
            }
            hashed = (unsigned)LW;
        } else if (chunked) {
            P2_TRY(absorb_upto(LW, true));  // what is left (the salts' chunks)
            P2_TRY(merkle_levels(ctx, geom, N));
        } else {
            P2_TRY(merkle_dev_impl(ctx, d_lde.u(), 0, N, LW, log_N, cap_height, 0, N, d_dig.u(), d_cap.u(), hash_n));
        }
        if (leaves_out && LW && !leaves_first && !early_transpose) P2_TRY(transpose_rows(ctx, d_lde.u(), N, LW, N, d_leaves.u(), leaf_rev));
        // coefficient blocks go back while the leaf sponge runs: queued behind the uploads on the copy stream, each
        // waiting for its block's transform only
        if (coeffs_out)
            for (size_t b = 0; b < nb; ++b) {
                const size_t c0 = blk0[b], cnt = blk0[b + 1] - c0;
                if (two_streams) P2_HIP(ctx, hipStreamWaitEvent(ctx->side, done[b], 0));
                if (coeffs_cols) {
                    for (size_t c = c0; c < c0 + cnt; ++c)
                        P2_HIP(ctx, hipMemcpyAsync(coeffs_cols[c], d_work.u() + c * n, n * 8, hipMemcpyDeviceToHost, copy_stream));
                } else {
                    P2_HIP(ctx, hipMemcpyAsync(coeffs_out + c0 * n, d_work.u() + c0 * n, cnt * n * 8, hipMemcpyDeviceToHost, copy_stream));
                }
            }
        if (leaves_out && LW && async_leaves) {
            // (issued above, right after the transposition; the later blocks follow the digests below)
        } else if (leaves_out && LW) {
            hipStream_t ls = ctx->stream;
            if (leaves_ev) {
                P2_HIP(ctx, hipStreamWaitEvent(copy_stream, leaves_ev, 0));
                ls = copy_stream;
            }
            P2_HIP(ctx, hipMemcpyAsync(leaves_out, d_leaves.p, LW * N * 8, hipMemcpyDeviceToHost, ls));
        }
        if (digests_out && nd && tail_groups > 1) {  // the groups' digest slices, each behind its group's levels only
            const size_t cnt = N / tail_groups, sub_leaves = N >> cap_height, sub_words = 8 * (sub_leaves - 1);
            for (size_t g = 0; g < tail_groups; ++g) {
                const size_t w0 = (g * cnt / sub_leaves) * sub_words, nw = (cnt / sub_leaves) * sub_words;
                if (two_streams) P2_HIP(ctx, hipStreamWaitEvent(copy_stream, tail_ev[g], 0));
                P2_HIP(ctx, hipMemcpyAsync(digests_out + w0, d_dig.u() + w0, nw * 8, hipMemcpyDeviceToHost, copy_stream));
            }
        } else if (digests_out && nd) {
            P2_HIP(ctx, hipMemcpyAsync(digests_out, d_dig.p, nd * 32, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (leafcopy && leafcopy->ev.size() < N / leafcopy->rows_per_block) {  // the rest of the leaf blocks, behind the digests' copy
            hipEvent_t e;
            P2_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            leafcopy->aux2 = e;
            P2_HIP(ctx, hipEventRecord(e, tail_groups > 1 ? copy_stream : ctx->stream));
            P2_HIP(ctx, hipStreamWaitEvent(ctx->leaf_stream, e, 0));
            P2_TRY(issue_leaf_blocks(leafcopy->ev.size(), N / leafcopy->rows_per_block));
        }
        if (cap_out) P2_TRY(d2h(ctx, cap_out, d_cap.p, cap_words * 8));
        return P2HOT_OK;
    };
    int rc = body();
    ctx->stream = main_stream;
    hipError_t e1 = hipSuccess;
    if (two_streams) e1 = hipStreamSynchronize(ctx->side);
    if (xsplit && ctx->xform_stream) {
        hipError_t e2 = hipStreamSynchronize(ctx->xform_stream);
        if (e1 == hipSuccess) e1 = e2;
    }
    for (hipEvent_t ev : lde_ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : up) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : done) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : tail_ev) (void)hipEventDestroy(ev);
    if (leaves_ev) (void)hipEventDestroy(leaves_ev);
    rc = sync_checked(ctx, rc, "commit");
    if (rc == P2HOT_OK && e1 != hipSuccess) P2_FAIL(ctx, P2HOT_EHIP, "commit: %s", hipGetErrorString(e1));
    if (rc == P2HOT_OK && handle_out) {
        *handle_out = make_batch(ctx, d_lde, d_dig, d_work, keep_vals ? &d_vals : nullptr, W, log_n, rate_bits, cap_height, S);
        (*handle_out)->hash_n = hash_n;
    }
    if (leafcopy) {
        if (rc == P2HOT_OK && handle_out && *handle_out) {
            leafcopy->d_staging = d_leaves.p;  // stays alive behind the handle until the last block has landed
            d_leaves.p = nullptr;
            (*handle_out)->leafcopy = leafcopy;
        } else {  // a failed call leaves nothing in flight
            (void)hipStreamSynchronize(ctx->leaf_stream);
            for (hipEvent_t ev : leafcopy->ev) (void)hipEventDestroy(ev);
            if (leafcopy->aux) (void)hipEventDestroy(leafcopy->aux);
            if (leafcopy->aux2) (void)hipEventDestroy(leafcopy->aux2);
            delete leafcopy;
        }
    }
    return rc;
}

static void leafcopy_finish(p2hot_batch *b) {  // waits for the copy in flight and returns its staging block
    if (!b || !b->leafcopy) return;
    // this batch's copy only: the leaf stream is the context's, and a later batch's 9 GB may be queued behind this one's.  The
    // block events are recorded in stream order, so the last one covers every block and both auxiliary waits
    const p2hot_batch::LeafCopy *lc = b->leafcopy;
    if (!lc->ev.empty() && lc->rows_per_block && lc->ev.size() == lc->rows / lc->rows_per_block)
        (void)hipEventSynchronize(lc->ev.back());
    else if (b->ctx->leaf_stream)
        (void)hipStreamSynchronize(b->ctx->leaf_stream);  // (a copy that was never fully issued: nothing else to wait on)
    for (hipEvent_t ev : b->leafcopy->ev) (void)hipEventDestroy(ev);
    if (b->leafcopy->aux) (void)hipEventDestroy(b->leafcopy->aux);
    if (b->leafcopy->aux2) (void)hipEventDestroy(b->leafcopy->aux2);
    pool_release(b->ctx, b->leafcopy->d_staging);
    delete b->leafcopy;
    b->leafcopy = nullptr;
}

// LOCK-FREE (rayon workers call it while another thread is inside a locked p2hot_* call of the same context): it therefore
// never writes the context's error text -- the code is all a failure reports
extern "C" int p2hot_batch_leaves_wait(p2hot_batch *b, size_t row_lo, size_t row_hi) {
    if (!b) return P2HOT_EINVAL;
    if (row_lo > row_hi || row_hi > b->N) return P2HOT_EINVAL;
    if (!b->leafcopy || row_lo == row_hi) return P2HOT_OK;
    DeviceGuard dev_guard_(b->ctx);
    const size_t rpb = b->leafcopy->rows_per_block;
    for (size_t k = row_lo / rpb; k <= (row_hi - 1) / rpb; ++k)
        if (hipEventSynchronize(b->leafcopy->ev[k]) != hipSuccess) return P2HOT_EHIP;
    return P2HOT_OK;
}
// rows per block of the pending asynchronous leaf copy (min(64, N / 1024) blocks, at least one), 0 when nothing is in flight:
// once row r has landed, so has every row below (r / rows_per_block + 1) * rows_per_block -- what the shim rounds its mark up to
extern "C" size_t p2hot_batch_leaves_block_rows(const p2hot_batch *b) { return b && b->leafcopy ? b->leafcopy->rows_per_block : 0; }

extern "C" int p2hot_commit(p2hot_ctx *ctx, const uint64_t *const *cols, size_t W, unsigned log_n, unsigned rate_bits,
                            unsigned cap_height, int is_values, unsigned flags, uint64_t *coeffs_out, uint64_t *leaves_out,
                            uint64_t *digests_out, uint64_t *cap_out, p2hot_batch **handle_out) {
    return commit_host(ctx, cols, W, log_n, rate_bits, cap_height, is_values, flags, nullptr, 0, coeffs_out, leaves_out, digests_out,
                       cap_out, handle_out);
}

extern "C" int p2hot_commit_salted(p2hot_ctx *ctx, const uint64_t *const *cols, size_t W, unsigned log_n, unsigned rate_bits,
                                   unsigned cap_height, int is_values, unsigned flags, const uint64_t *const *salt_cols,
                                   size_t n_salt, uint64_t *coeffs_out, uint64_t *leaves_out, uint64_t *digests_out,
                                   uint64_t *cap_out, p2hot_batch **handle_out) {
    return commit_host(ctx, cols, W, log_n, rate_bits, cap_height, is_values, flags, salt_cols, n_salt, coeffs_out, leaves_out,
                       digests_out, cap_out, handle_out);
}

// from_values / from_coeffs on a device-resident column set.  CONSUMES `cols` -- its block becomes the batch's coefficients
// (from_coeffs) or its kept values (from_values with P2HOT_KEEP_VALUES), or is released -- on success and on every failure
// EXCEPT P2HOT_EBUSY (another call is running on the context) and P2HOT_EINVAL (a null set, a set of another context, a borrowed
// view, an empty set, a bad rate / cap height / flag word): every argument is validated before the set is touched, so those two
// codes always mean "not consumed, the caller still owns the handle".
extern "C" int p2hot_commit_cols(p2hot_ctx *ctx, p2hot_cols *cols, unsigned rate_bits, unsigned cap_height, int is_values,
                                 unsigned flags, uint64_t *coeffs_out, uint64_t *leaves_out, uint64_t *digests_out,
                                 uint64_t *cap_out, p2hot_batch **handle_out) {
    P2_ENTER(ctx);
    if (handle_out) *handle_out = nullptr;
    if (!cols) P2_FAIL(ctx, P2HOT_EINVAL, "commit_cols: null column set");
    // every argument is checked BEFORE the set is touched: any P2HOT_EINVAL (and P2HOT_EBUSY) means "not consumed"
    if (cols->ctx != ctx || !cols->owned) P2_FAIL(ctx, P2HOT_EINVAL, "commit_cols: the column set belongs to another context or is a borrowed view");
    const size_t W = cols->W;
    const unsigned log_n = cols->log_n;
    P2_TRY(check_log(ctx, log_n + rate_bits, "commit_cols"));
    if (W == 0) P2_FAIL(ctx, P2HOT_EINVAL, "commit_cols: no polynomials (the reference panics on polynomials[0], fri/oracle.rs:90)");
    if (flags & ~(unsigned)(P2HOT_KEEP_VALUES | P2HOT_COEFFS_PER_COLUMN | P2HOT_HASH_MASK))
        P2_FAIL(ctx, P2HOT_EINVAL, "commit_cols: unknown flags %#x", flags);
    const unsigned hash_n = (flags & P2HOT_HASH_MASK) >> 8;
    if (hash_n) P2_TRY(check_hash_size(ctx, hash_n, "commit_cols"));
    uint64_t *const *coeffs_cols = (flags & P2HOT_COEFFS_PER_COLUMN) ? reinterpret_cast<uint64_t *const *>(coeffs_out) : nullptr;
    if (coeffs_cols)
        for (size_t c = 0; c < W; ++c)
            if (!coeffs_cols[c]) P2_FAIL(ctx, P2HOT_EINVAL, "commit_cols: coefficient destination %zu is null", c);
    const size_t n = (size_t)1 << log_n, N = n << rate_bits;
    const unsigned log_N = log_n + rate_bits;
    if (cap_height > log_N) P2_FAIL(ctx, P2HOT_EINVAL, "commit_cols: cap_height %u > log2(N) %u (merkle_tree.rs:195-200)", cap_height, log_N);
    // everything that can be refused for its ARGUMENTS is refused before the consume point, so that "EINVAL / EBUSY = not consumed"
    // (include/p2hot.h) holds for nested checks too: the transforms launch one grid row per polynomial (65535 at most)
    if (W > 65535) P2_FAIL(ctx, P2HOT_EINVAL, "commit_cols: %zu polynomials exceed the launch grid (65535 per call)", W);
    PoolBuf d_in(ctx);
    d_in.p = cols->d;
    delete cols;  // consumed from here on: the block is ours whatever happens below
    const size_t nd = p2hot_num_digests(log_N, cap_height), cap_words = (size_t)4 << cap_height;
    const bool keep_vals = is_values && handle_out && (flags & P2HOT_KEEP_VALUES);
    PoolBuf d_coef(ctx), d_lde(ctx), d_leaves(ctx), d_dig(ctx), d_cap(ctx);
    const size_t Wn = (W ? W : 1) * n * 8, WN = (W ? W : 1) * N * 8;
    if (keep_vals) P2_TRY(pool_alloc(ctx, Wn, &d_coef.p));
    P2_TRY(pool_alloc(ctx, WN, &d_lde.p));
    if (leaves_out) P2_TRY(pool_alloc(ctx, WN, &d_leaves.p));
    P2_TRY(pool_alloc(ctx, (nd ? nd : 1) * 32, &d_dig.p));
    P2_TRY(pool_alloc(ctx, cap_words * 8, &d_cap.p));
    auto body = [&]() -> int {
        u64 *co = d_in.u();
        if (keep_vals) {
            P2_HIP(ctx, hipMemcpyAsync(d_coef.p, d_in.p, W * n * 8, hipMemcpyDeviceToDevice, ctx->stream));
            co = d_coef.u();
        }
        if (is_values) {
            P2_TRY(ntt_natural(ctx, co, W, n, log_n, true));
        } else if (W) {
            P2HOT_LAUNCH(ntt::canon_kernel, dim3(cdiv(W * n, 256)), dim3(256), 0, ctx->stream, co, W * n);
            P2_LAUNCH_CHECK(ctx);
        }
        P2_TRY(commit_dev_impl(ctx, co, n, W, log_n, rate_bits, cap_height, 0, 0, N, nullptr, 0, d_lde.u(), N,
                               leaves_out ? d_leaves.u() : nullptr, d_dig.u(), d_cap.u(), hash_n));
        if (coeffs_cols) {
            for (size_t c = 0; c < W; ++c) P2_HIP(ctx, hipMemcpyAsync(coeffs_cols[c], co + c * n, n * 8, hipMemcpyDeviceToHost, ctx->stream));
        } else if (coeffs_out && W) {
            P2_HIP(ctx, hipMemcpyAsync(coeffs_out, co, W * n * 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (leaves_out && W) P2_HIP(ctx, hipMemcpyAsync(leaves_out, d_leaves.p, W * N * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (digests_out && nd) P2_HIP(ctx, hipMemcpyAsync(digests_out, d_dig.p, nd * 32, hipMemcpyDeviceToHost, ctx->stream));
        if (cap_out) P2_TRY(d2h(ctx, cap_out, d_cap.p, cap_words * 8));
        return P2HOT_OK;
    };
    int rc = sync_checked(ctx, body(), "commit_cols");
    if (rc == P2HOT_OK && handle_out) {
        if (keep_vals)
            *handle_out = make_batch(ctx, d_lde, d_dig, d_coef, &d_in, W, log_n, rate_bits, cap_height);
        else
            *handle_out = make_batch(ctx, d_lde, d_dig, d_in, nullptr, W, log_n, rate_bits, cap_height);
        (*handle_out)->hash_n = hash_n;
    }
    return rc;
}

// ------------------------------------------------------------------ M commitments of one shape in one set of launches
// Recursion-size proofs (2^12 rows) are latency-bound: a tree level is one ~12 us permutation chain whatever its width.  M
// proofs of the same shape therefore share every launch: their columns are interleaved as [W][M][n] (column e of all proofs,
// then column e+1, ...), so the iNTT and the coset LDE see W*M polynomials, and the M leaf matrices form ONE forest of
// M * 2^cap_height subtrees (leaf L = m*N + r of width W, column stride M*N): the digest array is the M trees' arrays back to back,
// the cap array the M caps -- exactly what M separate p2hot_commit_dev calls produce (fri/oracle.rs:57-112 per proof).
// the argument checks every commit_many form shares; `polys` = W * M
static int commit_many_check(p2hot_ctx *ctx, size_t M, size_t polys, unsigned log_N, unsigned cap_height) {
    if (polys == 0) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: no polynomials (the reference panics on polynomials[0], fri/oracle.rs:90)");
    if (M & (M - 1)) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: the number of proofs (%zu) must be a power of two", M);
    if (cap_height > log_N) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: cap_height %u > log2(N) %u (merkle_tree.rs:195-200)", cap_height, log_N);
    if (polys > 65535) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: W * M = %zu polynomials exceed one launch (65535)", polys);
    return P2HOT_OK;
}

extern "C" int p2hot_commit_many_dev(p2hot_ctx *ctx, uint64_t *d_cols, size_t M, size_t W, unsigned log_n, unsigned rate_bits,
                                     unsigned cap_height, int is_values, uint64_t *d_lde, uint64_t *d_digests, uint64_t *d_cap) {
    if (!ctx) return P2HOT_EINVAL;
    DeviceGuard dev_guard_(ctx);
    P2_TRY(check_log(ctx, log_n + rate_bits, "commit_many"));
    if (M == 0) return P2HOT_OK;
    const unsigned log_N = log_n + rate_bits;
    P2_TRY(commit_many_check(ctx, M, W * M, log_N, cap_height));
    unsigned lm = 0;
    while (((size_t)1 << lm) < M) ++lm;
    if (!d_cols || !d_lde || !d_cap || (p2hot_num_digests(log_N, cap_height) && !d_digests)) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: null buffer");
    const size_t n = (size_t)1 << log_n, N = n << rate_bits;
    if (is_values) {
        P2_TRY(ntt_natural(ctx, d_cols, W * M, n, log_n, true));  // "IFFT": in place, the block becomes the coefficients
    } else {
        P2HOT_LAUNCH(ntt::canon_kernel, dim3(cdiv(W * M * n, 256)), dim3(256), 0, ctx->stream, d_cols, W * M * n);
        P2_LAUNCH_CHECK(ctx);
    }
    P2_TRY(p2hot_coset_lde_dev(ctx, d_cols, W * M, n, log_n, rate_bits, gl::COSET_SHIFT, 0, N, d_lde, N));
    // one forest: M * 2^cap_height subtrees of 2^(log_N - cap_height) leaves
    return p2hot_merkle_dev(ctx, d_lde, 0, M * N, W, log_N + lm, cap_height + lm, 0, M * N, d_digests, d_cap);
}

// what both host forms do once the interleaved block d_co [W][M][n] is theirs: LDE, forest and caps in one set of launches, one
// synchronisation, then one p2hot_batch per proof -- shares of the blocks, freed with the last handle.  `cols` (p2hot_commit_many):
// host columns, interleaved on the way in: column e of proof m lands in slot e * M + m (one staged copy for short columns)
static int commit_many_core(p2hot_ctx *ctx, const char *what, PoolBuf &d_co, const uint64_t *const *cols, size_t M, size_t W, unsigned log_n,
                            unsigned rate_bits, unsigned cap_height, int is_values, uint64_t *coeffs_out, uint64_t *digests_out,
                            uint64_t *caps_out, p2hot_batch **handles_out) {
    const unsigned log_N = log_n + rate_bits;
    const size_t n = (size_t)1 << log_n, N = n << rate_bits, nd = p2hot_num_digests(log_N, cap_height), cap_words = (size_t)4 << cap_height;
    PoolBuf d_lde(ctx), d_dig(ctx), d_cap(ctx);
    P2_TRY(pool_alloc(ctx, W * M * N * 8, &d_lde.p));
    P2_TRY(pool_alloc(ctx, (nd ? nd : 1) * M * 32, &d_dig.p));
    P2_TRY(pool_alloc(ctx, cap_words * M * 8, &d_cap.p));
    auto body = [&]() -> int {
        if (cols) {
            std::vector<const uint64_t *> order(W * M);
            for (size_t e = 0; e < W; ++e)
                for (size_t m = 0; m < M; ++m) order[e * M + m] = cols[m * W + e];
            P2_TRY(h2d_columns(ctx, d_co.u(), order.data(), W * M, n * 8, 0, W * M * n * 8, ctx->stream));
        }
        P2_TRY(p2hot_commit_many_dev(ctx, d_co.u(), M, W, log_n, rate_bits, cap_height, is_values, d_lde.u(), d_dig.u(), d_cap.u()));
        if (coeffs_out)  // [M][W][n] <- [W][M][n]: one strided copy per proof
            for (size_t m = 0; m < M; ++m) P2_TRY(d2h_2d(ctx, coeffs_out + m * W * n, n * 8, d_co.u() + m * n, M * n * 8, n * 8, W));
        if (digests_out && nd) P2_TRY(d2h(ctx, digests_out, d_dig.p, nd * M * 32));
        if (caps_out) P2_TRY(d2h(ctx, caps_out, d_cap.p, cap_words * M * 8));
        return P2HOT_OK;
    };
    int rc = sync_checked(ctx, body(), what);
    if (rc != P2HOT_OK || !handles_out) return rc;
    SharedBlocks *sh = new SharedBlocks;
    sh->refs = (int)M;
    sh->lde = d_lde.p, sh->dig = d_dig.p, sh->coef = d_co.p;
    for (size_t m = 0; m < M; ++m) {
        p2hot_batch *b = new p2hot_batch{ctx, d_lde.u() + m * N, W, N, d_dig.u() + m * nd * 4, log_N, cap_height};
        b->d_coef = d_co.u() + m * n;
        b->log_n = log_n;
        b->rate_bits = rate_bits;
        b->lde_stride = M * N;
        b->coef_stride = M * n;
        b->shared = sh;
        handles_out[m] = b;
    }
    d_lde.p = d_dig.p = d_co.p = nullptr;  // owned by the handles now
    return rc;
}

// the host-pointer form: cols[m * W + e] = column e of proof m (n words each).  coeffs_out [M][W][n], digests_out [M][nd][4],
// caps_out [M][2^cap_height][4] (any may be NULL); handles_out [M] (optional): one p2hot_batch per proof, for p2hot_batch_rows /
// _paths / _coeffs, p2hot_eval_openings and p2hot_prove_openings -- they share the device blocks, freed with the last handle.
extern "C" int p2hot_commit_many(p2hot_ctx *ctx, const uint64_t *const *cols, size_t M, size_t W, unsigned log_n, unsigned rate_bits,
                                 unsigned cap_height, int is_values, uint64_t *coeffs_out, uint64_t *digests_out, uint64_t *caps_out,
                                 p2hot_batch **handles_out) {
    P2_ENTER(ctx);
    if (handles_out)
        for (size_t m = 0; m < M; ++m) handles_out[m] = nullptr;
    P2_TRY(check_log(ctx, log_n + rate_bits, "commit_many"));
    if (M == 0) return P2HOT_OK;
    P2_TRY(commit_many_check(ctx, M, W * M, log_n + rate_bits, cap_height));
    if (!cols) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: null column table");
    for (size_t i = 0; i < M * W; ++i)
        if (!cols[i]) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: column %zu of proof %zu is null", i % W, i / W);
    PoolBuf d_co(ctx);
    P2_TRY(pool_alloc(ctx, (W * M * 8) << log_n, &d_co.p));
    return commit_many_core(ctx, "commit_many", d_co, cols, M, W, log_n, rate_bits, cap_height, is_values, coeffs_out, digests_out, caps_out, handles_out);
}

// p2hot_commit_many for a device column set that is already interleaved ([W][M][n]: p2hot_partial_products_many's,
// p2hot_quotient_polys_gates_many's); the set is consumed
extern "C" int p2hot_commit_cols_many(p2hot_ctx *ctx, p2hot_cols *cols, size_t M, unsigned rate_bits, unsigned cap_height, int is_values,
                                      uint64_t *caps_out, p2hot_batch **handles_out) {
    P2_ENTER(ctx);
    if (handles_out)
        for (size_t m = 0; m < M; ++m) handles_out[m] = nullptr;
    if (M == 0) return P2HOT_OK;  // nothing done, nothing consumed
    // every argument is checked BEFORE the set is touched: P2HOT_EINVAL (and P2HOT_EBUSY) mean "not consumed" (p2hot_commit_cols' rule)
    if (!cols) P2_FAIL(ctx, P2HOT_EINVAL, "commit_cols_many: null column set");
    if (cols->ctx != ctx || !cols->owned) P2_FAIL(ctx, P2HOT_EINVAL, "commit_cols_many: the column set belongs to another context or is a borrowed view");
    const unsigned log_n = cols->log_n, log_N = log_n + rate_bits;
    P2_TRY(check_log(ctx, log_N, "commit_cols_many"));
    P2_TRY(commit_many_check(ctx, M, cols->W, log_N, cap_height));
    if (cols->W % M) P2_FAIL(ctx, P2HOT_EINVAL, "commit_cols_many: a set of %zu columns is not an interleaved set of %zu proofs", cols->W, M);
    unsigned lm = 0;
    while (((size_t)1 << lm) < M) ++lm;
    P2_TRY(check_log(ctx, log_N + lm, "commit_cols_many"));
    const size_t W = cols->W / M;
    PoolBuf d_co(ctx);
    d_co.p = cols->d;
    delete cols;  // consumed from here on: the block is ours whatever happens below
    return commit_many_core(ctx, "commit_cols_many", d_co, nullptr, M, W, log_n, rate_bits, cap_height, is_values, nullptr, nullptr, caps_out, handles_out);
}

// a handle over device buffers the caller owns (the *_dev flow: p2hot_commit_dev outputs); nothing is copied or freed
extern "C" int p2hot_batch_wrap_dev(p2hot_ctx *ctx, const uint64_t *d_coeffs, const uint64_t *d_lde, const uint64_t *d_digests,
                                    size_t W, unsigned log_n, unsigned rate_bits, unsigned cap_height, p2hot_batch **out) {
    if (!ctx || !out) return P2HOT_EINVAL;
    *out = nullptr;
    P2_TRY(check_log(ctx, log_n + rate_bits, "batch_wrap"));
    if (cap_height > log_n + rate_bits) P2_FAIL(ctx, P2HOT_EINVAL, "batch_wrap: cap_height > log2(N)");
    if (W && (!d_coeffs || !d_lde)) P2_FAIL(ctx, P2HOT_EINVAL, "batch_wrap: null buffer");
    if (p2hot_num_digests(log_n + rate_bits, cap_height) && !d_digests) P2_FAIL(ctx, P2HOT_EINVAL, "batch_wrap: null digests");
    p2hot_batch *b = new p2hot_batch{ctx, (u64 *)d_lde, W, ((size_t)1 << log_n) << rate_bits, (u64 *)d_digests, log_n + rate_bits, cap_height};
    b->d_coef = (u64 *)d_coeffs;
    b->log_n = log_n;
    b->rate_bits = rate_bits;
    b->owned = false;
    *out = b;
    return P2HOT_OK;
}

extern "C" size_t p2hot_batch_width(const p2hot_batch *b) { return b ? b->W : 0; }
extern "C" size_t p2hot_batch_leaf_width(const p2hot_batch *b) { return b ? b->W + b->S : 0; }
extern "C" unsigned p2hot_batch_degree_log(const p2hot_batch *b) { return b ? b->log_n : 0; }

// the kept input values of a from_values batch as a BORROWED column set (valid while the batch lives; free the view
// with p2hot_cols_free, which leaves the batch's block alone)
extern "C" int p2hot_batch_values(p2hot_batch *b, p2hot_cols **out) {
    if (!b || !out) return P2HOT_EINVAL;
    *out = nullptr;
    if (!b->d_vals) P2_FAIL(b->ctx, P2HOT_EINVAL, "batch_values: the batch was not committed with P2HOT_KEEP_VALUES");
    *out = new p2hot_cols{b->ctx, b->d_vals, b->W, b->log_n, false};
    return P2HOT_OK;
}

// polynomials [first, first + count) of the batch as VALUES on the subgroup H_n (an owned column set): a forward NTT of a copy of
// their device-resident coefficients.  What plonk/prover.rs reads as `prover_data.sigmas` (the sigma polynomials' values, row
// by row: prover.rs:413) is this for the sigma range of the constants_sigmas commitment -- the input of p2hot_partial_products.
extern "C" int p2hot_batch_subgroup_values(p2hot_batch *b, size_t first, size_t count, p2hot_cols **out) {
    if (!b || !out) return P2HOT_EINVAL;
    p2hot_ctx *ctx = b->ctx;
    P2_ENTER(ctx);
    *out = nullptr;
    if (first > b->W || count > b->W - first || count == 0) P2_FAIL(ctx, P2HOT_EINVAL, "batch_subgroup_values: polynomials [%zu,+%zu) of %zu", first, count, b->W);
    const size_t n = (size_t)1 << b->log_n;
    PoolBuf d(ctx);
    P2_TRY(pool_alloc(ctx, count * n * 8, &d.p));
    auto body = [&]() -> int {
        P2_HIP(ctx, hipMemcpy2DAsync(d.p, n * 8, b->d_coef + first * b->col_stride_coef(), b->col_stride_coef() * 8, n * 8, count,
                                     hipMemcpyDeviceToDevice, ctx->stream));
        P2_TRY(p2hot_fft_dev(ctx, d.u(), count, n, b->log_n));
        P2HOT_LAUNCH(ntt::canon_kernel, dim3(cdiv(count * n, 256)), dim3(256), 0, ctx->stream, d.u(), count * n);
        P2_LAUNCH_CHECK(ctx);
        return P2HOT_OK;
    };
    int rc = sync_checked(ctx, body(), "batch_subgroup_values");
    if (rc != P2HOT_OK) return rc;
    *out = new p2hot_cols{ctx, d.u(), count, b->log_n, true};
    d.p = nullptr;
    return P2HOT_OK;
}

extern "C" int p2hot_batch_coeffs(p2hot_batch *b, size_t first, size_t count, uint64_t *out) {
    if (!b) return P2HOT_EINVAL;
    p2hot_ctx *ctx = b->ctx;
    P2_ENTER(ctx);
    if (first > b->W || count > b->W - first) P2_FAIL(ctx, P2HOT_EINVAL, "batch_coeffs: polynomials [%zu,+%zu) of %zu", first, count, b->W);
    if (count == 0) return P2HOT_OK;
    if (!out) P2_FAIL(ctx, P2HOT_EINVAL, "batch_coeffs: null output");
    const size_t n = (size_t)1 << b->log_n;
    PoolBuf tmp(ctx);
    P2_TRY(pool_alloc(ctx, count * n * 8, &tmp.p));
    P2_HIP(ctx, hipMemcpy2DAsync(tmp.p, n * 8, b->d_coef + first * b->col_stride_coef(), b->col_stride_coef() * 8, n * 8, count,
                                 hipMemcpyDeviceToDevice, ctx->stream));
    P2HOT_LAUNCH(ntt::canon_kernel, dim3(cdiv(count * n, 256)), dim3(256), 0, ctx->stream, tmp.u(), count * n);
    P2_LAUNCH_CHECK(ctx);
    P2_HIP(ctx, hipMemcpyAsync(out, tmp.p, count * n * 8, hipMemcpyDeviceToHost, ctx->stream));
    return sync_checked(ctx, P2HOT_OK, "batch_coeffs");
}

extern "C" int p2hot_batch_digests(p2hot_batch *b, uint64_t *out) {
    if (!b) return P2HOT_EINVAL;
    p2hot_ctx *ctx = b->ctx;
    P2_ENTER(ctx);
    const size_t nd = p2hot_num_digests(b->log_N, b->cap_height);
    if (nd == 0) return P2HOT_OK;
    if (!out) P2_FAIL(ctx, P2HOT_EINVAL, "batch_digests: null output");
    P2_HIP(ctx, hipMemcpyAsync(out, b->d_dig, nd * 32, hipMemcpyDeviceToHost, ctx->stream));
    return sync_checked(ctx, P2HOT_OK, "batch_digests");
}

extern "C" int p2hot_batch_rows(p2hot_batch *b, const uint64_t *row_idx, size_t m, uint64_t *out) {
    if (!b) return P2HOT_EINVAL;
    p2hot_ctx *ctx = b->ctx;
    P2_ENTER(ctx);
    const size_t LW = b->W + b->S;  // MerkleTree::get returns the whole leaf, salt included (get_lde_values strips it, oracle.rs:146)
    if (m == 0 || LW == 0) return P2HOT_OK;
    if (!row_idx || !out) P2_FAIL(ctx, P2HOT_EINVAL, "batch_rows: null buffer");
    for (size_t i = 0; i < m; ++i)
        if (row_idx[i] >= b->N) P2_FAIL(ctx, P2HOT_EINVAL, "batch_rows: index %llu out of range", (unsigned long long)row_idx[i]);
    PoolBuf d_idx(ctx), d_out(ctx);
    P2_TRY(pool_alloc(ctx, m * 8, &d_idx.p));
    P2_TRY(pool_alloc(ctx, m * LW * 8, &d_out.p));
    auto body = [&]() -> int {
        P2_HIP(ctx, hipMemcpyAsync(d_idx.p, row_idx, m * 8, hipMemcpyHostToDevice, ctx->stream));
        P2_TRY(p2hot_gather_rows_dev(ctx, b->d_lde, b->col_stride_lde(), b->N, LW, d_idx.u(), m, d_out.u()));
        P2_TRY(d2h(ctx, out, d_out.p, m * LW * 8));
        return P2HOT_OK;
    };
    return sync_checked(ctx, body(), "batch_rows");
}

extern "C" int p2hot_batch_paths(p2hot_batch *b, const uint64_t *leaf_idx, size_t m, uint64_t *out) {
    if (!b) return P2HOT_EINVAL;
    p2hot_ctx *ctx = b->ctx;
    P2_ENTER(ctx);
    const unsigned layers = b->log_N - b->cap_height;
    if (m == 0 || layers == 0) return P2HOT_OK;
    if (!leaf_idx || !out) P2_FAIL(ctx, P2HOT_EINVAL, "batch_paths: null buffer");
    for (size_t i = 0; i < m; ++i)
        if (leaf_idx[i] >= b->N) P2_FAIL(ctx, P2HOT_EINVAL, "batch_paths: index %llu out of range", (unsigned long long)leaf_idx[i]);
    PoolBuf d_idx(ctx), d_out(ctx);
    P2_TRY(pool_alloc(ctx, m * 8, &d_idx.p));
    P2_TRY(pool_alloc(ctx, m * layers * 32, &d_out.p));
    auto body = [&]() -> int {
        P2_HIP(ctx, hipMemcpyAsync(d_idx.p, leaf_idx, m * 8, hipMemcpyHostToDevice, ctx->stream));
        P2_TRY(p2hot_merkle_paths_dev(ctx, b->d_dig, b->log_N, b->cap_height, d_idx.u(), m, d_out.u()));
        P2_TRY(d2h(ctx, out, d_out.p, m * layers * 32));
        return P2HOT_OK;
    };
    return sync_checked(ctx, body(), "batch_paths");
}

extern "C" void p2hot_batch_free(p2hot_batch *b) {
    if (!b) return;
    leafcopy_finish(b);  // P2HOT_LEAVES_ASYNC: the caller's buffer is complete (and the staging block idle) when this returns
    if (b->shared) {  // a member of a batched commitment: the last one returns the blocks
        if (b->shared->refs.fetch_sub(1) == 1) {
            (void)hipStreamSynchronize(b->ctx->stream);
            pool_release(b->ctx, b->shared->lde);
            pool_release(b->ctx, b->shared->dig);
            pool_release(b->ctx, b->shared->coef);
            delete b->shared;
        }
    } else if (b->owned) {
        (void)hipStreamSynchronize(b->ctx->stream);
        pool_release(b->ctx, b->d_lde);
        pool_release(b->ctx, b->d_dig);
        pool_release(b->ctx, b->d_coef);
        pool_release(b->ctx, b->d_vals);
    }
    delete b;
}

// returns the cached free blocks of the host-pointer entry points to the driver (the cache is grow-only otherwise)
extern "C" int p2hot_ctx_trim(p2hot_ctx *ctx) {
    P2_ENTER(ctx);
    P2_HIP(ctx, stream_sync(ctx));
    {
        std::lock_guard<std::mutex> pool_lock_(ctx->pool_mu);
        for (auto &blk : ctx->pool_free) (void)hipFree(blk.first);
        ctx->pool_free.clear();
        for (auto &blk : ctx->host_pool_free) (void)hipHostFree(blk.first);
        ctx->host_pool_free.clear();
    }
    // the per-size L_0 denominator tables of p2hot_quotient_polys (8 bytes per point of the quotient coset: 64 MB at 2^20 gates);
    // rebuilt in 0.35 ms by the next call that needs one
    for (auto it = ctx->twid_cache.begin(); it != ctx->twid_cache.end();) {
        if (std::get<0>(it->first) == 100) {
            (void)hipFree(it->second);
            it = ctx->twid_cache.erase(it);
        } else {
            ++it;
        }
    }
    for (p2hot_ctx *h : ctx->helpers) {  // the sibling contexts of p2hot_prove_openings_many keep their own block caches
        P2_HIP(ctx, stream_sync(h));
        std::lock_guard<std::mutex> pool_lock_(h->pool_mu);
        for (auto &blk : h->pool_free) (void)hipFree(blk.first);
        h->pool_free.clear();
    }
    return P2HOT_OK;
}

// ------------------------------------------------------------------ OpeningSet::new (plonk/proof.rs:314-327)
// What prove_openings needs to know about an oracle: its coefficient polynomials on THIS context, and -- when the tree
// lives on this context too -- its LDE matrix and digest array.  d_lde == NULL: the rows and paths of the initial trees
// are served elsewhere (a sharded batch: by the rank that owns the row) through `open_initial`.
struct OracleView {
    const u64 *d_coef, *d_lde, *d_dig;
    size_t W, N;
    size_t S = 0;  // salt columns behind the W polynomial columns of d_lde (blinded oracles): a leaf is W + S words
    size_t lde_stride = 0, coef_stride = 0;  // elements between columns when they are interleaved with other proofs' (0: N / n)
    size_t leaf_width() const { return W + S; }
    size_t col_lde() const { return lde_stride ? lde_stride : N; }
    size_t col_coef(unsigned log_n) const { return coef_stride ? coef_stride : ((size_t)1 << log_n); }
};
static OracleView view_of(const p2hot_batch *B) {
    return OracleView{B->d_coef, B->d_lde, B->d_dig, B->W, B->N, B->S, B->lde_stride, B->coef_stride};
}
// How prove_openings_core opens the initial trees; exactly one of the two is given.
// DeviceOpener: enqueues, for oracle o and the Q query indices at d_idx, the rows [Q][leaf width] and the paths [Q][layers][4]
typedef std::function<int(size_t o, const u64 *d_idx, size_t Q, u64 *d_rows, u64 *d_paths)> DeviceOpener;
// InitialOpener: fills proof->initial_leaves / initial_paths (query-major layout) for the Q host-resident query indices, after
// the synchronisation that ends the device work
typedef std::function<int(const u64 *idx, size_t Q, u64 *leaves_out, u64 *paths_out)> InitialOpener;

// OpeningSet::new for oracles given as views: a device table of pointers to every polynomial in order, one
// p2hot_eval_polys_dev call, then per-oracle copies into the caller's layout ([n_points][W_o][2] per oracle)
static int eval_openings_core(p2hot_ctx *ctx, const std::vector<OracleView> &views, unsigned log_n, const uint64_t *points, size_t n_points,
                              uint64_t *out);

extern "C" int p2hot_eval_openings(p2hot_ctx *ctx, const p2hot_batch *const *batches, size_t n_batches, const uint64_t *points,
                                   size_t n_points, uint64_t *out) {
    P2_ENTER(ctx);
    if (n_batches == 0 || n_points == 0) return P2HOT_OK;
    if (!batches || !points || !out) P2_FAIL(ctx, P2HOT_EINVAL, "eval_openings: null argument");
    std::vector<OracleView> views;
    for (size_t b = 0; b < n_batches; ++b) {
        const p2hot_batch *B = batches[b];
        if (!B || B->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "oracle %zu is null or belongs to another context", b);
        if (B->log_n != batches[0]->log_n)
            P2_FAIL(ctx, P2HOT_EINVAL, "all oracles must have the same degree (oracle %zu: 2^%u vs 2^%u)", b, B->log_n, batches[0]->log_n);
        views.push_back(view_of(B));
    }
    return eval_openings_core(ctx, views, batches[0]->log_n, points, n_points, out);
}

// the device pointer of every polynomial of every oracle, in order; `grp` (the M-form): the proof each belongs to, `per_proof` oracles each
static void opening_table(const std::vector<OracleView> &views, unsigned log_n, std::vector<const u64 *> &ptrs,
                          std::vector<unsigned> *grp = nullptr, size_t per_proof = 1) {
    for (size_t o = 0; o < views.size(); ++o)
        for (size_t j = 0; j < views[o].W; ++j) {
            ptrs.push_back(views[o].d_coef + j * views[o].col_coef(log_n));
            if (grp) grp->push_back((unsigned)(o / per_proof));
        }
}

// host copies from the evaluation layout [n_points][total][2] into the caller's: per oracle [n_points][W_o][2], the oracles back to back
static void openings_scatter(const std::vector<OracleView> &views, const std::vector<u64> &res, size_t n_points, uint64_t *out) {
    const size_t total = res.size() / (2 * n_points);
    size_t off = 0, out_off = 0;
    for (auto &v : views) {
        for (size_t p = 0; p < n_points; ++p)
            std::copy(res.begin() + 2 * (p * total + off), res.begin() + 2 * (p * total + off + v.W), out + out_off + 2 * p * v.W);
        off += v.W;
        out_off += 2 * n_points * v.W;
    }
}

static int eval_openings_core(p2hot_ctx *ctx, const std::vector<OracleView> &views, unsigned log_n, const uint64_t *points, size_t n_points,
                              uint64_t *out) {
    std::vector<const u64 *> ptrs;
    opening_table(views, log_n, ptrs);
    const size_t total = ptrs.size();
    if (total == 0) return P2HOT_OK;
    PoolBuf d_table(ctx), d_res(ctx), d_out(ctx);
    P2_TRY(pool_alloc(ctx, total * sizeof(u64 *), &d_table.p));
    P2_TRY(pool_alloc(ctx, n_points * total * 16, &d_res.p));
    const bool one_copy = views.size() <= 8 && total <= 0xFFFFFFFFull;
    if (one_copy) P2_TRY(pool_alloc(ctx, n_points * total * 16, &d_out.p));
    auto body = [&]() -> int {
        P2_HIP(ctx, hipMemcpyAsync(d_table.p, ptrs.data(), total * sizeof(u64 *), hipMemcpyHostToDevice, ctx->stream));
        // device layout [n_points][total][2]; the caller's layout is per oracle [n_points][W_o][2]
        P2_TRY(p2hot_eval_polys_dev(ctx, (const uint64_t *const *)d_table.p, total, log_n, points, n_points, d_res.u()));
        if (one_copy) {  // reordered on the device, one copy back (each copy into pageable memory costs ~20 us of host time)
            fri::OpeningLayout lay{};
            lay.n_oracles = (unsigned)views.size();
            size_t first = 0;
            for (size_t o = 0; o < views.size(); ++o) {
                lay.width[o] = (unsigned)views[o].W;
                lay.first[o] = (unsigned)first;
                first += views[o].W;
            }
            P2HOT_LAUNCH(fri::reorder_openings_kernel, dim3(cdiv(n_points * total, 256)), dim3(256), 0, ctx->stream, (const u64 *)d_res.u(),
                         total, n_points, lay, d_out.u());
            P2_LAUNCH_CHECK(ctx);
            P2_TRY(d2h(ctx, out, d_out.p, n_points * total * 16));
            return P2HOT_OK;
        }
        size_t off = 0, out_off = 0;
        for (auto &v : views) {
            for (size_t p = 0; p < n_points && v.W; ++p)
                P2_HIP(ctx, hipMemcpyAsync(out + out_off + 2 * p * v.W, d_res.u() + 2 * (p * total + off), v.W * 16, hipMemcpyDeviceToHost,
                                           ctx->stream));
            off += v.W;
            out_off += 2 * n_points * v.W;
        }
        return P2HOT_OK;
    };
    return sync_checked(ctx, body(), "eval_openings");  // `ptrs` outlives the copy: the stream is idle on return
}

// OpeningSet::new for M proofs of n_batches oracles each, every proof at its own n_points points: one launch per stage for all of them
extern "C" int p2hot_eval_openings_many(p2hot_ctx *ctx, size_t M, const p2hot_batch *const *batches, size_t n_batches, const uint64_t *points,
                                        size_t n_points, uint64_t *out) {
    P2_ENTER(ctx);
    const char *what = "eval_openings_many";
    if (M == 0 || n_batches == 0 || n_points == 0) return P2HOT_OK;
    if (!batches || !points || !out) P2_FAIL(ctx, P2HOT_EINVAL, "%s: null argument", what);
    if (M > 0x7FFFFFFFull / n_batches) P2_FAIL(ctx, P2HOT_EINVAL, "%s: too many oracles", what);
    std::vector<OracleView> views;
    for (size_t j = 0; j < M; ++j)
        for (size_t b = 0; b < n_batches; ++b) {
            const p2hot_batch *B = batches[j * n_batches + b];
            if (!B || B->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "%s: proof %zu: oracle %zu is null or belongs to another context", what, j, b);
            if (B->log_n != batches[0]->log_n)
                P2_FAIL(ctx, P2HOT_EINVAL, "%s: proof %zu: all oracles must have the same degree (oracle %zu: 2^%u vs 2^%u)", what, j, b, B->log_n,
                        batches[0]->log_n);
            views.push_back(view_of(B));
        }
    const unsigned log_n = batches[0]->log_n;
    P2_TRY(check_log(ctx, log_n, what));
    // every polynomial of every proof in order, with the proof it belongs to
    std::vector<const u64 *> ptrs;
    std::vector<unsigned> grp;
    opening_table(views, log_n, ptrs, &grp, n_batches);
    const size_t total = ptrs.size();
    if (total == 0) return P2HOT_OK;
    const size_t n = (size_t)1 << log_n;
    const unsigned seg_log = log_n < 12 ? log_n : 12;  // p2hot_eval_polys_dev's segments
    const size_t n_seg = n >> seg_log, seg = (size_t)1 << seg_log, G = M * n_points;
    if (total > 0x7FFFFFFFull || n_seg > 65535 || n_points > 65535 || G > 65535) P2_FAIL(ctx, P2HOT_EINVAL, "%s: too many polynomials, points or proofs for one launch", what);
    // host blob: pointers [total] | proof of polynomial [total] (u32) | points [G][2] | (z^seg, (z^seg)^256) [G][4]
    const size_t o_grp = total, o_pts = o_grp + (total + 1) / 2, o_zs = o_pts + 2 * G, blob_words = o_zs + 4 * G;
    std::vector<u64> blob(blob_words);
    std::copy(ptrs.begin(), ptrs.end(), reinterpret_cast<const u64 **>(blob.data()));
    std::copy(grp.begin(), grp.end(), reinterpret_cast<unsigned *>(blob.data() + o_grp));
    for (size_t g = 0; g < G; ++g) {
        const gl::ext2 z{gl::canon(points[2 * g]), gl::canon(points[2 * g + 1])};
        const gl::ext2 zs = ext_pow(z, (u64)1 << seg_log), zs256 = ext_pow(zs, 256);
        blob[o_pts + 2 * g] = z.a0, blob[o_pts + 2 * g + 1] = z.a1;
        blob[o_zs + 4 * g] = gl::canon(zs.a0), blob[o_zs + 4 * g + 1] = gl::canon(zs.a1);
        blob[o_zs + 4 * g + 2] = gl::canon(zs256.a0), blob[o_zs + 4 * g + 3] = gl::canon(zs256.a1);
    }
    PoolBuf d_blob(ctx), d_w(ctx), d_part(ctx), d_res(ctx);
    P2_TRY(pool_alloc(ctx, blob_words * 8, &d_blob.p));
    P2_TRY(pool_alloc(ctx, G * 2 * seg * 8, &d_w.p));
    P2_TRY(pool_alloc(ctx, n_points * total * n_seg * 16, &d_part.p));
    P2_TRY(pool_alloc(ctx, n_points * total * 16, &d_res.p));
    std::vector<u64> res(n_points * total * 2);  // device layout [n_points][total][2]
    auto body = [&]() -> int {
        P2_HIP(ctx, hipMemcpyAsync(d_blob.p, blob.data(), blob_words * 8, hipMemcpyHostToDevice, ctx->stream));
        const u64 *const *d_ptrs = reinterpret_cast<const u64 *const *>(d_blob.u());
        const unsigned *d_grp = reinterpret_cast<const unsigned *>(d_blob.u() + o_grp);
        ProfScope ps(ctx, "eval_polys_many");
        P2HOT_LAUNCH(fri::ext_powers_many_kernel, dim3(cdiv(seg, 256), (unsigned)G), dim3(256), 0, ctx->stream, (const u64 *)(d_blob.u() + o_pts),
                     (unsigned)seg, d_w.u());
        P2HOT_LAUNCH(fri::eval_polys_dot_many_kernel, dim3((unsigned)total, (unsigned)n_seg, (unsigned)n_points), dim3(256), 0, ctx->stream, d_ptrs,
                     d_grp, seg_log, (const u64 *)d_w.u(), d_part.u());
        P2HOT_LAUNCH(fri::eval_polys_stage2_many_kernel, dim3((unsigned)total, (unsigned)n_points), dim3(256), 0, ctx->stream, (const u64 *)d_part.u(),
                     d_grp, n_seg, (const u64 *)(d_blob.u() + o_zs), d_res.u());
        P2_LAUNCH_CHECK(ctx);
        P2_HIP(ctx, hipMemcpyAsync(res.data(), d_res.p, res.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        return P2HOT_OK;
    };
    int rc = sync_checked(ctx, body(), what);
    if (rc != P2HOT_OK) return rc;
    openings_scatter(views, res, n_points, out);  // per proof p2hot_eval_openings' layout, the proofs back to back
    return P2HOT_OK;
}

// ------------------------------------------------------------------ prove_openings + fri_proof
static int fri_check_params(p2hot_ctx *ctx, const p2hot_fri_params *fp, unsigned log_n, FriRounds *rounds) {
    if (!fp) P2_FAIL(ctx, P2HOT_EINVAL, "null fri params");
    if (fp->n_reduction_rounds && !fp->reduction_arity_bits) P2_FAIL(ctx, P2HOT_EINVAL, "null reduction_arity_bits");
    P2_TRY(check_log(ctx, log_n + fp->rate_bits, "fri"));
    return fri_rounds(ctx, "fri", log_n, fp->rate_bits, fp->cap_height, fp->reduction_arity_bits, fp->n_reduction_rounds, rounds);
}

// sizes of the flat FriProof buffers for oracles of the given widths (include/p2hot.h, p2hot_fri_proof)
static int fri_proof_layout(const size_t *widths, size_t n_oracles, unsigned log_n, const p2hot_fri_params *fp, p2hot_fri_proof_layout *out) {
    if (!out || !fp || n_oracles == 0 || (fp->n_reduction_rounds && !fp->reduction_arity_bits)) return P2HOT_EINVAL;
    const unsigned log_N = log_n + fp->rate_bits;
    size_t w_sum = 0;
    for (size_t o = 0; o < n_oracles; ++o) w_sum += widths[o];
    const size_t q = fp->num_query_rounds, cap_words = (size_t)4 << fp->cap_height;
    FriRounds rounds;
    P2_TRY(fri_rounds(nullptr, nullptr, log_n, fp->rate_bits, fp->cap_height, fp->reduction_arity_bits, fp->n_reduction_rounds, &rounds));
    if (rounds.log_last < fp->rate_bits || log_N < fp->cap_height) return P2HOT_EINVAL;
    out->caps_words = fp->n_reduction_rounds * cap_words;
    out->final_poly_words = (size_t)2 << (rounds.log_last - fp->rate_bits);
    out->initial_leaves_words = q * w_sum;
    out->initial_paths_words = q * n_oracles * 4 * (size_t)(log_N - fp->cap_height);
    out->step_evals_words = q * rounds.ev_words;
    out->step_paths_words = q * rounds.pa_words;
    return P2HOT_OK;
}

extern "C" int p2hot_fri_proof_sizes(const p2hot_batch *const *oracles, size_t n_oracles, const p2hot_fri_params *fp,
                                     p2hot_fri_proof_layout *out) {
    if (!oracles || n_oracles == 0 || !oracles[0]) return P2HOT_EINVAL;
    std::vector<size_t> widths;
    for (size_t o = 0; o < n_oracles; ++o) {
        if (!oracles[o]) return P2HOT_EINVAL;
        widths.push_back(oracles[o]->W + oracles[o]->S);  // evals_proofs carry whole leaves (fri/prover.rs:238-241)
    }
    return fri_proof_layout(widths.data(), n_oracles, oracles[0]->log_n, fp, out);
}

static int prove_openings_views(p2hot_ctx *ctx, const p2hot_fri_batch_info *batches, size_t n_batches, const std::vector<OracleView> &views,
                                unsigned log_n, p2hot_challenger *challenger, const p2hot_fri_params *fp, p2hot_fri_proof *proof,
                                const InitialOpener *open_initial);

extern "C" int p2hot_prove_openings(p2hot_ctx *ctx, const p2hot_fri_batch_info *batches, size_t n_batches,
                                    const p2hot_batch *const *oracles, size_t n_oracles, p2hot_challenger *challenger,
                                    const p2hot_fri_params *fp, p2hot_fri_proof *proof) {
    P2_ENTER(ctx);
    if (!oracles || n_oracles == 0) P2_FAIL(ctx, P2HOT_EINVAL, "prove_openings: null argument");
    std::vector<OracleView> views;
    for (size_t o = 0; o < n_oracles; ++o) {
        if (!oracles[o] || oracles[o]->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "prove_openings: oracle %zu is null or belongs to another context", o);
        // Challenger<F, C::Hasher> (fri/oracle.rs:180): one hasher for the transcript and every tree.  Refused before any HIP call.
        if (challenger && oracles[o]->hash_n != challenger->hash_n) {
            if (!challenger->hash_n)
                P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "prove_openings: oracle %zu is a KeccakHash<%u> tree and the challenger a Poseidon one (create it with "
                        "p2hot_challenger_create_keccak)", o, oracles[o]->hash_n);
            if (!oracles[o]->hash_n)
                P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "prove_openings: oracle %zu is a Poseidon tree and the challenger a KeccakHash<%u> one", o,
                        challenger->hash_n);
            P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "prove_openings: oracle %zu is a KeccakHash<%u> tree and the challenger a KeccakHash<%u> one", o,
                    oracles[o]->hash_n, challenger->hash_n);
        }
        if (oracles[o]->log_n != oracles[0]->log_n || (fp && (oracles[o]->rate_bits != fp->rate_bits || oracles[o]->cap_height != fp->cap_height)))
            P2_FAIL(ctx, P2HOT_EINVAL, "prove_openings: oracle %zu was committed with another degree / rate / cap height", o);
        views.push_back(view_of(oracles[o]));
    }
    return prove_openings_views(ctx, batches, n_batches, views, oracles[0]->log_n, challenger, fp, proof, nullptr);
}

// ------------------------------------------------------------------ M opening proofs side by side
// A recursion-size opening proof (2^12 rows) is a chain of small launches -- about 36 dependent challenger permutations, tree
// levels of a few hundred nodes -- that leaves the chip almost idle.  M independent proofs therefore run on up to 4 sibling
// contexts of the same GPU (their own streams, scratch and block caches), each driven by its own host thread, so that the
// launches of different proofs overlap on the device.  Every proof is computed by the same prove_openings_views as a single
// p2hot_prove_openings call: results are identical, buffer by buffer.
static int helper_contexts(p2hot_ctx *ctx, size_t want) {
    while (ctx->helpers.size() < want) {
        hipStream_t st = nullptr;
        P2_HIP(ctx, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        p2hot_ctx *h = nullptr;
        int rc = p2hot_ctx_create(ctx->device, (void *)st, &h);
        if (rc != P2HOT_OK) {
            ctx->err = std::string("prove_openings_many: helper context: ") + (h ? h->err : "allocation failed");
            if (h) p2hot_ctx_destroy(h);
            return rc;
        }
        p2hot_challenger *hc = nullptr;
        rc = p2hot_challenger_create(h, &hc);
        if (rc != P2HOT_OK) {
            ctx->err = "prove_openings_many: helper challenger: " + h->err;
            p2hot_ctx_destroy(h);
            return rc;
        }
        ctx->helpers.push_back(h);
        ctx->helper_streams.push_back(st);
        ctx->helper_challengers.push_back(hc);
    }
    // the parent's tuning knobs and profiling switch as they are NOW (p2hot_tune_* / p2hot_profile_enable may have been called
    // since the helpers were made)
    for (p2hot_ctx *h : ctx->helpers) {
        h->quad_threshold = ctx->quad_threshold;
        h->row_threshold = ctx->row_threshold;
        h->use_regpass = ctx->use_regpass;
        h->use_limb = ctx->use_limb;
        h->ntt_radix_bits = ctx->ntt_radix_bits;
        h->overlap = ctx->overlap;
        h->horner_two_level_min = ctx->horner_two_level_min;
        h->profiling = ctx->profiling;
    }
    return P2HOT_OK;
}

// ------------------------------------------------------------------ M opening proofs of one shape in one set of launches
// "One shape": distinct Poseidon transcripts and Poseidon oracles (the caller has refused Keccak), the same number of batches, the same
// (oracle_index, poly_index) lists in every batch -- the points are per proof -- and the same polynomial and salt widths per oracle
// position.  Anything else (a list that names a polynomial which does not exist included) takes the side-by-side path, which reports it.
static bool many_one_shape(size_t M, const p2hot_fri_batch_info *const *batches, const size_t *n_batches,
                           const std::vector<std::vector<OracleView>> &views, p2hot_challenger *const *challengers) {
    std::set<const p2hot_challenger *> seen;
    for (size_t j = 0; j < M; ++j) {
        if (!seen.insert(challengers[j]).second) return false;
        if (n_batches[j] != n_batches[0] || (n_batches[j] && !batches[j])) return false;
        for (size_t o = 0; o < views[j].size(); ++o)
            if (views[j][o].W != views[0][o].W || views[j][o].S != views[0][o].S) return false;
        for (size_t i = 0; i < n_batches[j]; ++i) {
            const p2hot_fri_batch_info &a = batches[0][i], &b = batches[j][i];
            if (b.n_polys != a.n_polys || (b.n_polys && (!b.oracle_index || !b.poly_index))) return false;
            for (size_t k = 0; k < b.n_polys; ++k) {
                if (b.oracle_index[k] != a.oracle_index[k] || b.poly_index[k] != a.poly_index[k]) return false;
                if (j == 0 && (b.oracle_index[k] >= views[0].size() || b.poly_index[k] >= views[0][b.oracle_index[k]].W)) return false;
            }
        }
    }
    return true;
}

// PolynomialBatch::prove_openings + fri_proof (fri/oracle.rs:176-237, fri/prover.rs:24-82) for M proofs of one shape: every launch
// of prove_openings_core once per GROUP of proofs (fri_many_group), the proof on a grid axis, on the caller's context and stream.
// Per group: alpha_j, the final polynomials as planes [2][g][n], the commit phase (the round trees of a round are one forest), the
// grind, the witness and the query indices, then the rows and paths of the g oracles of each oracle position and of the g round
// trees of each round, written query-major into one staging block -- a proof's four query buffers as p2hot.h lays them out -- that
// one copy brings to a pinned block.  The groups reuse the device blocks in stream order; ONE synchronisation ends the call and the
// host scatters the staging into the callers' buffers.  Everything is validated before the first enqueue.
// A proof whose device-searched grind range held no witness (probability e^-32) gets its transcript back as it was before the call
// and is proved again alone, by the single-proof path with its host-checked grind; the other proofs of the call stand.
static int prove_openings_many_core(p2hot_ctx *ctx, size_t M, const p2hot_fri_batch_info *const *batches, size_t n_batches,
                                    const std::vector<std::vector<OracleView>> &views, unsigned log_n, p2hot_challenger *const *challengers,
                                    const p2hot_fri_params *fp, p2hot_fri_proof *proofs) {
    const char *what = "prove_openings_many";
    FriRounds rounds;
    P2_TRY(fri_check_params(ctx, fp, log_n, &rounds));
    const unsigned rate_bits = fp->rate_bits, cap_height = fp->cap_height, log_N = log_n + rate_bits, R = fp->n_reduction_rounds;
    const size_t Q = fp->num_query_rounds, n = (size_t)1 << log_n, N = n << rate_bits, n_oracles = views[0].size();
    if (R > 32) P2_FAIL(ctx, P2HOT_EINVAL, "%s: more than 32 reduction rounds", what);
    if (fp->proof_of_work_bits > 64) P2_FAIL(ctx, P2HOT_EINVAL, "%s: proof_of_work_bits > 64", what);
    std::vector<size_t> leaf_widths;
    size_t w_sum = 0;
    for (auto &v : views[0]) {
        leaf_widths.push_back(v.leaf_width());
        w_sum += v.leaf_width();
    }
    p2hot_fri_proof_layout lay;
    if (fri_proof_layout(leaf_widths.data(), n_oracles, log_n, fp, &lay) != P2HOT_OK) P2_FAIL(ctx, P2HOT_EINVAL, "%s: inconsistent parameters", what);
    for (size_t j = 0; j < M; ++j) {
        const p2hot_fri_proof &pr = proofs[j];
        if ((lay.caps_words && !pr.commit_phase_merkle_caps) || !pr.final_poly ||
            (Q && ((lay.initial_leaves_words && !pr.initial_leaves) || (lay.initial_paths_words && !pr.initial_paths) ||
                   (lay.step_evals_words && !pr.step_evals) || (lay.step_paths_words && !pr.step_paths))))
            P2_FAIL(ctx, P2HOT_EINVAL, "%s: proof %zu: a proof buffer is null (size them with p2hot_fri_proof_sizes)", what, j);
    }
    // the polynomial table of the shared instance (FriInstanceInfo.batches, fri/structure.rs) and every proof's points
    std::vector<size_t> offsets(1, 0);
    for (size_t i = 0; i < n_batches; ++i) offsets.push_back(offsets.back() + batches[0][i].n_polys);
    const size_t total = offsets.back(), G = fri_many_group(M, log_N), idx_words = (1 + (size_t)R) * Q;
    const unsigned layers0 = log_N - cap_height;
    const size_t caps_words = lay.caps_words, final_words = lay.final_poly_words;
    // a proof's staging record: its four query buffers, query-major
    const size_t o_leaves = 0, o_paths = o_leaves + lay.initial_leaves_words, o_evals = o_paths + lay.initial_paths_words,
                 o_steps = o_evals + lay.step_evals_words, rec = Q ? o_steps + lay.step_paths_words : 0;
    PoolBuf d_small(ctx), d_planes(ctx), d_leaves(ctx), d_dig(ctx), d_q(ctx), d_save(ctx), fp_scratch(ctx), commit_scratch(ctx);
    P2_TRY(pool_alloc(ctx, 2 * G * n * 8, &d_planes.p));
    P2_TRY(pool_alloc(ctx, (rounds.leaf_words ? G * rounds.leaf_words : 1) * 8, &d_leaves.p));
    P2_TRY(pool_alloc(ctx, (rounds.dig_words ? G * rounds.dig_words : 1) * 8, &d_dig.p));
    P2_TRY(pool_alloc(ctx, M * sizeof(fri::Challenger), &d_save.p));
    // alpha [G][2] | witness [G] | response [G] | rand [G][Q] | idx [G][1 + R][Q] | staging [G][rec]
    P2_TRY(pool_alloc(ctx, G * (4 + Q + idx_words + rec) * 8, &d_q.p));
    u64 *q_alpha = d_q.u(), *q_best = q_alpha + 2 * G, *q_resp = q_best + G, *q_rand = q_resp + G, *q_idx = q_rand + G * Q, *q_stage = q_idx + G * idx_words;
    // one small upload: transcripts [M] | polynomial pointers [M][total] | initial trees [n_oracles][M] | round trees [R][G]
    static_assert(sizeof(fri::ManyTree) == 24 && sizeof(fri::Challenger *) == 8, "table words");
    const size_t s_tab = M, s_init = s_tab + M * total, s_round = s_init + 3 * n_oracles * M, small_words = s_round + 3 * (size_t)R * G;
    std::vector<u64> small(small_words), pts(2 * M * n_batches + 1), zt(6 * M * n_batches + 1);
    P2_TRY(pool_alloc(ctx, small_words * 8, &d_small.p));
    for (size_t j = 0; j < M; ++j) {
        small[j] = (u64)(uintptr_t)challengers[j]->d;
        u64 *tab = small.data() + s_tab + j * total;
        for (size_t i = 0, k = 0; i < n_batches; ++i) {
            const p2hot_fri_batch_info &bi = batches[j][i];
            for (size_t e = 0; e < bi.n_polys; ++e, ++k) {
                const OracleView &v = views[j][bi.oracle_index[e]];
                tab[k] = (u64)(uintptr_t)(v.d_coef + bi.poly_index[e] * v.col_coef(log_n));
            }
            pts[2 * (j * n_batches + i)] = bi.point[0];
            pts[2 * (j * n_batches + i) + 1] = bi.point[1];
        }
        for (size_t o = 0; o < n_oracles; ++o) {
            const OracleView &v = views[j][o];
            u64 *t = small.data() + s_init + 3 * (o * M + j);
            t[0] = (u64)(uintptr_t)v.d_lde, t[1] = (u64)(uintptr_t)v.d_dig, t[2] = v.col_lde();
        }
    }
    for (unsigned r = 0; r < R; ++r)
        for (size_t y = 0; y < G; ++y) {  // proof y of a group: its slice of the group's round trees
            u64 *t = small.data() + s_round + 3 * (r * G + y);
            t[0] = (u64)(uintptr_t)(d_leaves.u() + y * rounds.leaf_words + rounds.round[r].leaf_off);
            t[1] = (u64)(uintptr_t)(d_dig.u() + y * rounds.dig_words + rounds.round[r].dig_off);
            t[2] = 0;
        }
    fri::Challenger *const *d_chs = reinterpret_cast<fri::Challenger *const *>(d_small.u());
    const u64 *const *d_tables = reinterpret_cast<const u64 *const *>(d_small.u() + s_tab);
    const fri::ManyTree *d_init = reinterpret_cast<const fri::ManyTree *>(d_small.u() + s_init);
    const fri::ManyTree *d_round = reinterpret_cast<const fri::ManyTree *>(d_small.u() + s_round);
    fri::ArityBits ab{};
    for (unsigned r = 0; r < R; ++r) ab.b[r] = (unsigned char)rounds.round[r].arity_bits;
    // host landing blocks: the staging records and the query indices (pinned, one copy each per group), caps, final polynomials, witnesses
    struct Pinned {
        p2hot_ctx *ctx;
        void *p = nullptr;
        ~Pinned() { p2hot_host_free(ctx, p); }
    } h_block{ctx};
    P2_TRY(p2hot_host_alloc(ctx, (M * (rec + idx_words) + 1) * 8, &h_block.p));
    u64 *h_stage = (u64 *)h_block.p, *h_idx = h_stage + M * rec;
    std::vector<u64> h_caps(M * caps_words + 1), h_final(M * final_words + 1);
    std::vector<unsigned long long> best(M, ~0ull);
    auto group = [&](size_t j0, size_t g) -> int {
        const unsigned gy = (unsigned)g;
        fri::Challenger *const *chs = d_chs + j0;
        // oracle.rs:186: alpha_j = challenger_j.get_extension_challenge()
        P2_TRY(challenger_many_dev(ctx, chs, g, nullptr, 0, 0, q_alpha, 2, 2));
        // oracle.rs:190-213: the final polynomials, planes [2][g][n]
        P2_TRY(final_poly_many_core(ctx, g, d_tables + j0 * total, total, offsets.data(), n_batches, pts.data() + 2 * j0 * n_batches, q_alpha, 2, log_n,
                                    d_planes.u(), fp_scratch, zt.data() + 6 * j0 * n_batches));
        // oracle.rs:215-220 + fri/prover.rs:40-51: the commit phase; the round trees stay on the device, proof-major
        P2_TRY(fri_commit_many_core(ctx, g, d_planes.u(), log_n, rate_bits, cap_height, fp->reduction_arity_bits, R, fp->max_num_query_steps,
                                    fp->final_poly_coeff_len, chs, rounds.leaf_words ? d_leaves.u() : nullptr, rounds.dig_words ? d_dig.u() : nullptr,
                                    true, caps_words ? h_caps.data() + j0 * caps_words : nullptr, nullptr, h_final.data() + j0 * final_words,
                                    commit_scratch));
        // fri/prover.rs:53-58, :197-198: the grind, then observe the witness and draw the response
        u64 pow_next = 0;
        P2_TRY(pow_search_many_dev(ctx, chs, g, fp->proof_of_work_bits, (unsigned long long *)q_best, &pow_next));
        P2_TRY(challenger_many_dev(ctx, chs, g, q_best, 1, 1, q_resp, 1, 1));
        P2_TRY(d2h(ctx, best.data() + j0, q_best, g * 8));
        if (Q == 0) return P2HOT_OK;
        // fri/prover.rs:215-220, :243-253: the query indices
        P2_TRY(challenger_many_dev(ctx, chs, g, nullptr, 0, 0, q_rand, Q, Q));
        P2HOT_LAUNCH(fri::query_indices_many_kernel, dim3(cdiv(Q, 256), gy), dim3(256), 0, ctx->stream, (const u64 *)q_rand, Q, log_N, ab, R, q_idx);
        P2_LAUNCH_CHECK(ctx);
        // prover.rs:238-241: per oracle position (tree.get(x), tree.prove(x)) of the g oracles, all queries per launch
        size_t w_off = 0;
        for (size_t o = 0; o < n_oracles; ++o) {
            const fri::ManyTree *tr = d_init + o * M + j0;
            const size_t Wb = leaf_widths[o];
            if (Wb)
                P2HOT_LAUNCH(fri::gather_rows_many_kernel, dim3(cdiv(Q * Wb, 256), gy), dim3(256), 0, ctx->stream, tr, 1, Wb, N, (const u64 *)q_idx,
                             idx_words, Q, q_stage + o_leaves, rec, w_sum, w_off, ctx->d_oob);
            if (layers0)
                P2HOT_LAUNCH(fri::merkle_paths_many_kernel, dim3(cdiv(Q * layers0, 256), gy), dim3(256), 0, ctx->stream, tr, log_N, cap_height,
                             (const u64 *)q_idx, idx_words, Q, q_stage + o_paths, rec, n_oracles * 4 * layers0, o * 4 * layers0, ctx->d_oob);
            P2_LAUNCH_CHECK(ctx);
            w_off += Wb;
        }
        // prover.rs:242-253: per round (evals, tree.prove(x >> arity_bits)) of the g round trees
        for (unsigned r = 0; r < R; ++r) {
            const FriRound &f = rounds.round[r];
            const u64 *idx_r = q_idx + (1 + (size_t)r) * Q;
            P2HOT_LAUNCH(fri::gather_rows_many_kernel, dim3(cdiv(Q * f.ev_w, 256), gy), dim3(256), 0, ctx->stream, d_round + r * G, 0, f.ev_w,
                         f.rows >> f.arity_bits, idx_r, idx_words, Q, q_stage + o_evals, rec, rounds.ev_words, f.ev_off, ctx->d_oob);
            if (f.pa_w)
                P2HOT_LAUNCH(fri::merkle_paths_many_kernel, dim3(cdiv(Q * (f.pa_w / 4), 256), gy), dim3(256), 0, ctx->stream, d_round + r * G, f.log_leaves,
                             cap_height, idx_r, idx_words, Q, q_stage + o_steps, rec, rounds.pa_words, f.pa_off, ctx->d_oob);
            P2_LAUNCH_CHECK(ctx);
        }
        if (rec) P2_HIP(ctx, hipMemcpyAsync(h_stage + j0 * rec, q_stage, g * rec * 8, hipMemcpyDeviceToHost, ctx->stream));
        P2_HIP(ctx, hipMemcpyAsync(h_idx + j0 * idx_words, q_idx, g * idx_words * 8, hipMemcpyDeviceToHost, ctx->stream));
        return P2HOT_OK;
    };
    auto body = [&]() -> int {
        P2_HIP(ctx, hipMemcpyAsync(d_small.p, small.data(), small_words * 8, hipMemcpyHostToDevice, ctx->stream));
        // the transcripts as they arrive, for a proof that has to be proved again alone (see above)
        P2HOT_LAUNCH(fri::challenger_copy_many_kernel, dim3((unsigned)M), dim3(64), 0, ctx->stream, d_chs, (fri::Challenger *)d_save.p, 0);
        P2_LAUNCH_CHECK(ctx);
        for (size_t j0 = 0; j0 < M; j0 += G) P2_TRY(group(j0, std::min(G, M - j0)));
        return P2HOT_OK;
    };
    int rc = sync_checked(ctx, body(), what);
    if (rc != P2HOT_OK) return rc;
    for (size_t j = 0; j < M; ++j) {
        p2hot_fri_proof &pr = proofs[j];
        if (best[j] == ~0ull) {  // no witness in the device-searched range: this proof again, alone, from its transcript before the call
            P2HOT_LAUNCH(fri::challenger_copy_many_kernel, dim3(1), dim3(64), 0, ctx->stream, d_chs + j, (fri::Challenger *)d_save.p + j, 1);
            P2_LAUNCH_CHECK(ctx);
            int one = prove_openings_views(ctx, batches[j], n_batches, views[j], log_n, challengers[j], fp, &pr, nullptr);
            if (one != P2HOT_OK) {
                const std::string inner = ctx->err;
                P2_FAIL(ctx, one, "%s: proof %zu: %s", what, j, inner.c_str());
            }
            continue;
        }
        pr.pow_witness = best[j];
        if (caps_words) std::copy(h_caps.begin() + j * caps_words, h_caps.begin() + (j + 1) * caps_words, pr.commit_phase_merkle_caps);
        std::copy(h_final.begin() + j * final_words, h_final.begin() + (j + 1) * final_words, pr.final_poly);
        if (Q == 0) continue;
        const u64 *s = h_stage + j * rec;
        if (pr.query_indices) std::copy(h_idx + j * idx_words, h_idx + j * idx_words + Q, pr.query_indices);
        if (lay.initial_leaves_words) std::copy(s + o_leaves, s + o_paths, pr.initial_leaves);
        if (lay.initial_paths_words) std::copy(s + o_paths, s + o_evals, pr.initial_paths);
        if (lay.step_evals_words) std::copy(s + o_evals, s + o_steps, pr.step_evals);
        if (lay.step_paths_words) std::copy(s + o_steps, s + rec, pr.step_paths);
    }
    return P2HOT_OK;
}

extern "C" int p2hot_prove_openings_many(p2hot_ctx *ctx, size_t M, const p2hot_fri_batch_info *const *batches, const size_t *n_batches,
                                         const p2hot_batch *const *oracles, size_t n_oracles, p2hot_challenger *const *challengers,
                                         const p2hot_fri_params *fp, p2hot_fri_proof *proofs) {
    P2_ENTER(ctx);
    if (M == 0) return P2HOT_OK;
    if (!batches || !n_batches || !oracles || n_oracles == 0 || !challengers || !proofs) P2_FAIL(ctx, P2HOT_EINVAL, "prove_openings_many: null argument");
    std::vector<std::vector<OracleView>> views(M);
    for (size_t j = 0; j < M; ++j) {
        if (!challengers[j] || challengers[j]->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "prove_openings_many: challenger %zu is null or belongs to another context", j);
        if (challengers[j]->hash_n)  // (the helper contexts carry Poseidon transcripts)
            P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "prove_openings_many: challenger %zu is a KeccakHash<%u> transcript (Keccak opening proofs: p2hot_prove_openings, one at a time)",
                    j, challengers[j]->hash_n);
        for (size_t o = 0; o < n_oracles; ++o) {
            const p2hot_batch *B = oracles[j * n_oracles + o];
            if (!B || B->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "prove_openings_many: oracle %zu of proof %zu is null or belongs to another context", o, j);
            if (B->hash_n)
                P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "prove_openings_many: oracle %zu of proof %zu is a KeccakHash<%u> tree (Keccak opening proofs: p2hot_prove_openings, one at a time)",
                        o, j, B->hash_n);
            if (B->log_n != oracles[0]->log_n || (fp && (B->rate_bits != fp->rate_bits || B->cap_height != fp->cap_height)))
                P2_FAIL(ctx, P2HOT_EINVAL, "prove_openings_many: oracle %zu of proof %zu was committed with another degree / rate / cap height", o, j);
            views[j].push_back(view_of(B));
        }
    }
    // The fused path: proofs of one shape share every launch (prove_openings_many_core below).  P2HOT_MANY_FUSED, read per call
    // like P2HOT_MANY_HELPERS: 0 = always side by side; unset or 1 = fused where the proofs are eligible.
    {
        bool fused = true;
        if (const char *e = getenv("P2HOT_MANY_FUSED")) fused = atoi(e) != 0;
        if (fused && many_one_shape(M, batches, n_batches, views, challengers))
            return prove_openings_many_core(ctx, M, batches, n_batches[0], views, oracles[0]->log_n, challengers, fp, proofs);
    }
    size_t k_max = 4;  // sibling contexts: 2 and 4 measured 1.8-1.9x a single stream, 8+ no better (P2HOT_MANY_HELPERS overrides; tools/pom_trace.py)
    if (const char *e = getenv("P2HOT_MANY_HELPERS")) k_max = std::max<size_t>(1, std::min<size_t>(64, (size_t)strtoull(e, nullptr, 10)));
    const size_t K = std::min<size_t>(M, k_max);
    P2_TRY(helper_contexts(ctx, K));
    P2_HIP(ctx, stream_sync(ctx));  // the oracles and transcripts were produced on this context's stream
    const unsigned log_n = oracles[0]->log_n;
    std::vector<int> rcs(K, P2HOT_OK);
    std::vector<std::string> errs(K);
    auto work = [&](size_t k) {
        p2hot_ctx *h = ctx->helpers[k];
        p2hot_challenger *hc = ctx->helper_challengers[k];
        DeviceGuard dev_guard_(h);
        CallGuard guard_(h);
        for (size_t j = k; j < M && rcs[k] == P2HOT_OK; j += K) {
            auto one = [&]() -> int {
                P2_HIP(h, hipMemcpyAsync(hc->d, challengers[j]->d, sizeof(fri::Challenger), hipMemcpyDeviceToDevice, h->stream));
                P2_TRY(prove_openings_views(h, batches[j], n_batches[j], views[j], log_n, hc, fp, &proofs[j], nullptr));
                P2_HIP(h, hipMemcpyAsync(challengers[j]->d, hc->d, sizeof(fri::Challenger), hipMemcpyDeviceToDevice, h->stream));
                P2_HIP(h, stream_sync(h));
                return P2HOT_OK;
            };
            rcs[k] = one();
            if (rcs[k] != P2HOT_OK) errs[k] = "proof " + std::to_string(j) + ": " + h->err;
        }
    };
#ifdef P2HOT_EMU
    for (size_t k = 0; k < K; ++k) work(k);  // the kernel emulator is single-threaded
#else
    {
        std::vector<std::thread> th;
        for (size_t k = 1; k < K; ++k) th.emplace_back(work, k);
        work(0);
        for (auto &t : th) t.join();
    }
#endif
    if (ctx->profiling)  // the helpers' kernels belong to this call: their totals go to the parent's table
        for (size_t k = 0; k < K; ++k) {
            p2hot_ctx *h = ctx->helpers[k];
            (void)p2hot_profile_json(h, 0);  // drains h's recorded events into h->prof_acc
            for (auto &kv : h->prof_acc) {
                auto &acc = ctx->prof_acc[kv.first];
                acc.first += kv.second.first;
                acc.second += kv.second.second;
            }
            h->prof_acc.clear();
        }
    for (size_t k = 0; k < K; ++k)
        if (rcs[k] != P2HOT_OK) P2_FAIL(ctx, rcs[k], "prove_openings_many: %s", errs[k].c_str());
    return P2HOT_OK;
}

// ------------------------------------------------------------------ the opening proof: one core for plain, sharded and batch FRI
// One FRI instance (FriInstanceInfo, fri/structure.rs): the polynomials of one degree opened at each point, as device pointers in
// batch order.  The plain and sharded paths prove one instance; batch FRI one per degree, the largest first.
struct OpeningInstance {
    unsigned log_n = 0;
    std::vector<const u64 *> ptrs;
    std::vector<size_t> offsets = std::vector<size_t>(1, 0);  // batch b opens ptrs[offsets[b], offsets[b + 1])
    std::vector<u64> points;                                   // [n_batches][2]
    size_t n_batches() const { return offsets.size() - 1; }
};

// the query staging block of one proof, device words
struct QueryStaging {
    u64 *idx;                            // [1 + n_rounds][Q]: x_index, then x_index >> arity_bits per round
    u64 *leaves, *paths, *evals, *step_paths;  // the four query buffers of p2hot_fri_proof, oracle- / round-major
    u64 *rand, *alpha, *best, *resp;     // [Q] | [2] | PoW witness | PoW response
    u64 *chsave;                         // the transcript before the grind
};
static int query_staging_alloc(p2hot_ctx *ctx, size_t Q, unsigned n_rounds, const p2hot_fri_proof_layout &lay, PoolBuf *block, QueryStaging *s) {
    u64 **const member[] = {&s->idx, &s->leaves, &s->paths, &s->evals, &s->step_paths, &s->rand, &s->alpha, &s->best, &s->resp, &s->chsave};
    const size_t words[] = {Q * (1 + n_rounds), lay.initial_leaves_words, lay.initial_paths_words, lay.step_evals_words, lay.step_paths_words,
                            Q, 2, 1, 1, (sizeof(fri::Challenger) + 7) / 8};
    size_t total = 0;
    for (size_t w : words) total += w;
    P2_TRY(pool_alloc(ctx, total * 8, &block->p));
    u64 *p = block->u();
    for (size_t k = 0; k < sizeof words / sizeof *words; ++k) {
        *member[k] = p;
        p += words[k];
    }
    return P2HOT_OK;
}

// PolynomialBatch::prove_openings + fri_proof (fri/oracle.rs:176-237, fri/prover.rs:24-82) and their batch_fri counterparts
// (batch_fri/oracle.rs:128-192, batch_fri/prover.rs:25-86) after the caller's own validation.  `what` starts every error text.
// instances[0] has the largest degree and sets the proof's geometry; instances 1.. join the commit phase when the folded degree
// reaches theirs (the caller has checked that it does: batch_join_check).  leaf_widths: words of an initial leaf, per oracle.
static int prove_openings_core(p2hot_ctx *ctx, const char *what, const std::vector<OpeningInstance> &instances,
                               const std::vector<size_t> &leaf_widths, const DeviceOpener *open_device, const InitialOpener *open_host,
                               p2hot_challenger *challenger, const p2hot_fri_params *fp, p2hot_fri_proof *proof) {
    const size_t n_oracles = leaf_widths.size(), n_instances = instances.size();
    if (!challenger || challenger->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "%s: the challenger belongs to another context", what);
    if (!proof || n_instances == 0) P2_FAIL(ctx, P2HOT_EINVAL, "%s: null argument", what);
    // FriParams::hiding changes nothing on the prover's FRI path (it is observed into the transcript by the caller,
    // fri/mod.rs:148, and tells the VERIFIER to strip the salts, fri/verifier.rs:149-151): blinded oracles carry their salt columns
    const unsigned log_n = instances[0].log_n;
    FriRounds rounds;
    P2_TRY(fri_check_params(ctx, fp, log_n, &rounds));
    const unsigned rate_bits = fp->rate_bits, cap_height = fp->cap_height, log_N = log_n + rate_bits, n_rounds = fp->n_reduction_rounds;
    const size_t Q = fp->num_query_rounds;
    if (n_rounds > 32) P2_FAIL(ctx, P2HOT_EINVAL, "%s: more than 32 reduction rounds", what);
    if (fp->proof_of_work_bits > 64) P2_FAIL(ctx, P2HOT_EINVAL, "%s: proof_of_work_bits > 64", what);
    p2hot_fri_proof_layout lay;
    if (fri_proof_layout(leaf_widths.data(), n_oracles, log_n, fp, &lay) != P2HOT_OK) P2_FAIL(ctx, P2HOT_EINVAL, "%s: inconsistent parameters", what);
    if ((lay.caps_words && !proof->commit_phase_merkle_caps) || !proof->final_poly ||
        (Q && ((lay.initial_leaves_words && !proof->initial_leaves) || (lay.initial_paths_words && !proof->initial_paths) ||
               (lay.step_evals_words && !proof->step_evals) || (lay.step_paths_words && !proof->step_paths))))
        P2_FAIL(ctx, P2HOT_EINVAL, "%s: a proof buffer is null (size them with the *_fri_proof_sizes call of this path)", what);
    // --- device blocks: pointer tables, one final_poly plane pair per instance, round trees (leaves + digests), query staging
    size_t table_words = 0, plane_words = 0, w_sum = 0;
    for (auto &in : instances) {
        table_words += in.ptrs.size();
        plane_words += (size_t)2 << in.log_n;
    }
    for (size_t w : leaf_widths) w_sum += w;
    const unsigned layers0 = log_N - cap_height;
    PoolBuf d_table(ctx), d_planes(ctx), d_leaves(ctx), d_dig(ctx), d_q(ctx);
    QueryStaging q;
    P2_TRY(pool_alloc(ctx, (table_words ? table_words : 1) * sizeof(u64 *), &d_table.p));
    P2_TRY(pool_alloc(ctx, plane_words * 8, &d_planes.p));
    P2_TRY(pool_alloc(ctx, (rounds.leaf_words ? rounds.leaf_words : 1) * 8, &d_leaves.p));
    P2_TRY(pool_alloc(ctx, (rounds.dig_words ? rounds.dig_words : 1) * 8, &d_dig.p));
    P2_TRY(query_staging_alloc(ctx, Q, n_rounds, lay, &d_q, &q));
    fri::ArityBits ab{};
    for (unsigned r = 0; r < n_rounds; ++r) ab.b[r] = (unsigned char)rounds.round[r].arity_bits;
    std::vector<const uint64_t *> planes(n_instances);
    std::vector<unsigned> join_log_n;
    {
        u64 *p = d_planes.u();
        for (size_t i = 0; i < n_instances; ++i) {
            planes[i] = p;
            p += (size_t)2 << instances[i].log_n;
            if (i) join_log_n.push_back(instances[i].log_n);
        }
    }
    unsigned long long best = ~0ull;
    u64 pow_next = 0;
    std::vector<u64> idx_for_owners;
    // Everything below is enqueued without waiting for the GPU: alpha, beta_i, the PoW witness and the query indices
    // stay on the device (the challenger is device-resident), results reach the caller's buffers by asynchronous copies
    // and ONE synchronisation ends the call.
    auto head = [&]() -> int {
        // A copy from pageable host memory holds the host until the stream has drained.  The first instance's pointer table
        // therefore goes up before anything is launched (behind the challenger's kernel it would stall the enqueueing of a
        // launch-bound small proof); a joining instance's goes up immediately before its final_poly, where the wait hides
        // behind the previous instance's kernels.  Neither copy touches what the challenger reads: the order changes no result.
        const u64 **tab = (const u64 **)d_table.p;
        auto upload = [&](const OpeningInstance &in) -> int {
            if (!in.ptrs.empty())
                P2_HIP(ctx, hipMemcpyAsync(tab, in.ptrs.data(), in.ptrs.size() * sizeof(u64 *), hipMemcpyHostToDevice, ctx->stream));
            return P2HOT_OK;
        };
        P2_TRY(upload(instances[0]));
        // oracle.rs:186 (batch_fri/oracle.rs:138): alpha = challenger.get_extension_challenge(), once for every instance
        P2_TRY(challenger_step_dev(challenger, nullptr, 0, q.alpha, 2));
        // oracle.rs:190-213: final_poly = sum_i alpha^(k_i) (F_i - F_i(z_i)) / (X - z_i), one per instance (batch_fri/oracle.rs:143-179:
        // ReducingFactor's count is zero at the start of each, so every instance is the plain prelude with the same alpha)
        for (size_t i = 0; i < n_instances; ++i) {
            const OpeningInstance &in = instances[i];
            if (i) P2_TRY(upload(in));
            P2_TRY(final_poly_core(ctx, (const uint64_t *const *)tab, in.offsets.data(), in.n_batches(), in.points.data(), nullptr, q.alpha,
                                   in.log_n, (uint64_t *)planes[i]));
            tab += in.ptrs.size();
        }
        // oracle.rs:215-220 + fri/prover.rs:40-51 (batch_fri/prover.rs:53-62): final FFT, commit phase; the round trees stay on the device
        const BatchJoin join{planes.data() + 1, join_log_n.data(), n_instances - 1};
        P2_TRY(fri_commit_core(ctx, nullptr, planes[0], log_n, rate_bits, cap_height, fp->reduction_arity_bits, n_rounds,
                               fp->max_num_query_steps, fp->final_poly_coeff_len, challenger,
                               FriCommitOut{.leaves_out = d_leaves.u(), .leaves_on_device = true, .digests_out = d_dig.u(),
                                            .digests_on_device = true, .caps_out = proof->commit_phase_merkle_caps,
                                            .final_out = proof->final_poly, .defer_sync = true},
                               &join));
        // fri/prover.rs:53-58: proof of work, searched on the device; the transcript state before it is kept for the
        // (practically unreachable) case that the searched range holds no witness
        P2_HIP(ctx, hipMemcpyAsync(q.chsave, challenger->d, sizeof(fri::Challenger), hipMemcpyDeviceToDevice, ctx->stream));
        return pow_search_dev(ctx, challenger, fp->proof_of_work_bits, (unsigned long long *)q.best, &pow_next);
    };
    auto tail = [&]() -> int {
        // prover.rs:197-198: observe the witness, draw the response
        P2_TRY(challenger_step_dev(challenger, q.best, 1, q.resp, 1));
        P2_TRY(d2h(ctx, &best, q.best, 8));
        if (Q == 0) return P2HOT_OK;
        // fri/prover.rs:215-220: x_index = rand % n for num_query_rounds challenges; per round x_index >>= arity_bits (:243-253)
        P2_TRY(challenger_step_dev(challenger, nullptr, 0, q.rand, Q));
        P2HOT_LAUNCH(fri::query_indices_kernel, dim3(cdiv(Q, 256)), dim3(256), 0, ctx->stream, (const u64 *)q.rand, Q, log_N, ab, n_rounds,
                     q.idx);
        P2_LAUNCH_CHECK(ctx);
        if (proof->query_indices) P2_TRY(d2h(ctx, proof->query_indices, q.idx, Q * 8));
        if (open_host) {  // the owners of the rows need the indices on the host
            idx_for_owners.resize(Q);
            P2_TRY(d2h(ctx, idx_for_owners.data(), q.idx, Q * 8));
        }
        // prover.rs:238-241: initial_trees_proof = for every oracle (tree.get(x), tree.prove(x)), all queries per launch.
        // Device staging is oracle-major ([oracle][q][...]); the host layout is query-major (see p2hot.h), fixed by the D2H copies.
        size_t w_off = 0;
        for (size_t o = 0; o < n_oracles && open_device; ++o) {
            P2_TRY((*open_device)(o, q.idx, Q, q.leaves + Q * w_off, q.paths + o * Q * 4 * layers0));
            w_off += leaf_widths[o];
        }
        // prover.rs:242-253: per round (evals = unflatten(tree.get(x >> arity_bits)), tree.prove(x >> arity_bits))
        for (unsigned r = 0; r < n_rounds; ++r) {
            const FriRound &f = rounds.round[r];
            const u64 *d_idx_r = q.idx + (1 + (size_t)r) * Q;
            P2HOT_LAUNCH(fri::gather_rowmajor_kernel, dim3(cdiv(Q * f.ev_w, 256)), dim3(256), 0, ctx->stream,
                         (const u64 *)(d_leaves.u() + f.leaf_off), f.ev_w, f.rows >> f.arity_bits, d_idx_r, Q, q.evals + Q * f.ev_off, ctx->d_oob);
            P2_LAUNCH_CHECK(ctx);
            if (f.pa_w)
                P2_TRY(p2hot_merkle_paths_dev(ctx, d_dig.u() + f.dig_off, f.log_leaves, cap_height, d_idx_r, Q, q.step_paths + Q * f.pa_off));
        }
        // D2H: one strided copy per (oracle | round) turns the oracle-major staging into the query-major proof layout
        w_off = 0;
        for (size_t o = 0; o < n_oracles && open_device; ++o) {
            const size_t Wb = leaf_widths[o];
            if (Wb) P2_TRY(d2h_2d(ctx, proof->initial_leaves + w_off, w_sum * 8, q.leaves + Q * w_off, Wb * 8, Wb * 8, Q));
            if (layers0)
                P2_TRY(d2h_2d(ctx, proof->initial_paths + o * 4 * layers0, n_oracles * 4 * layers0 * 8, q.paths + o * Q * 4 * layers0,
                              4 * layers0 * 8, 4 * layers0 * 8, Q));
            w_off += Wb;
        }
        for (const FriRound &f : rounds.round) {
            P2_TRY(d2h_2d(ctx, proof->step_evals + f.ev_off, rounds.ev_words * 8, q.evals + Q * f.ev_off, f.ev_w * 8, f.ev_w * 8, Q));
            if (f.pa_w)
                P2_TRY(d2h_2d(ctx, proof->step_paths + f.pa_off, rounds.pa_words * 8, q.step_paths + Q * f.pa_off, f.pa_w * 8, f.pa_w * 8, Q));
        }
        return P2HOT_OK;
    };
    int rc = head();
    if (rc == P2HOT_OK) rc = tail();
    rc = sync_checked(ctx, rc, what);
    if (rc == P2HOT_OK && best == ~0ull) {
        // no witness among the first 2^(pow_bits + 5) candidates (probability e^-32): rewind the transcript to before the
        // grind, search the rest of the range with a host check per chunk, and replay the tail
        // (errors go through rc + sync_checked like the main path: the PoolBuf blocks must not return to the cache while
        // enqueued work still references them)
        auto fallback = [&]() -> int {
            P2_HIP(ctx, hipMemcpyAsync(challenger->d, q.chsave, sizeof(fri::Challenger), hipMemcpyDeviceToDevice, ctx->stream));
            P2_TRY(pow_continue_host(ctx, challenger, fp->proof_of_work_bits, (unsigned long long *)q.best, pow_next, &best));
            return tail();
        };
        rc = sync_checked(ctx, fallback(), what);
    }
    if (rc == P2HOT_OK) proof->pow_witness = best;
    // a sharded batch: the initial trees' rows and paths come from the ranks that own them
    if (rc == P2HOT_OK && open_host && Q) rc = (*open_host)(idx_for_owners.data(), Q, proof->initial_leaves, proof->initial_paths);
    return rc;
}

// One instance over oracles of one degree given as views: the plain path (the trees are on this context, open_initial == NULL)
// and the sharded one (open_initial serves the rows and paths from the ranks that own them).
static int prove_openings_views(p2hot_ctx *ctx, const p2hot_fri_batch_info *batches, size_t n_batches, const std::vector<OracleView> &views,
                                unsigned log_n, p2hot_challenger *challenger, const p2hot_fri_params *fp, p2hot_fri_proof *proof,
                                const InitialOpener *open_initial) {
    if (n_batches && !batches) P2_FAIL(ctx, P2HOT_EINVAL, "prove_openings: null argument");
    // the polynomial table of the instance (FriInstanceInfo.batches, fri/structure.rs): device pointers in batch order
    std::vector<OpeningInstance> instance(1);
    OpeningInstance &in = instance[0];
    in.log_n = log_n;
    for (size_t i = 0; i < n_batches; ++i) {
        const p2hot_fri_batch_info &bi = batches[i];
        if (bi.n_polys && (!bi.oracle_index || !bi.poly_index)) P2_FAIL(ctx, P2HOT_EINVAL, "prove_openings: batch %zu has null index arrays", i);
        for (size_t j = 0; j < bi.n_polys; ++j) {
            const size_t oi = bi.oracle_index[j], pi = bi.poly_index[j];
            if (oi >= views.size() || pi >= views[oi].W)
                P2_FAIL(ctx, P2HOT_EINVAL, "prove_openings: batch %zu opens polynomial (%zu, %zu) which does not exist", i, oi, pi);
            in.ptrs.push_back(views[oi].d_coef + pi * views[oi].col_coef(log_n));
        }
        in.offsets.push_back(in.ptrs.size());
        in.points.push_back(bi.point[0]);
        in.points.push_back(bi.point[1]);
    }
    std::vector<size_t> leaf_widths;
    for (auto &v : views) leaf_widths.push_back(v.leaf_width());
    const DeviceOpener on_device = [&](size_t o, const u64 *d_idx, size_t Q, u64 *d_rows, u64 *d_paths) -> int {
        const OracleView &B = views[o];
        P2_TRY(p2hot_gather_rows_dev(ctx, B.d_lde, B.col_lde(), B.N, B.leaf_width(), d_idx, Q, d_rows));
        return p2hot_merkle_paths_dev(ctx, B.d_dig, log_n + fp->rate_bits, fp->cap_height, d_idx, Q, d_paths);
    };
    return prove_openings_core(ctx, "prove_openings", instance, leaf_widths, open_initial ? nullptr : &on_device, open_initial, challenger,
                               fp, proof);
}
