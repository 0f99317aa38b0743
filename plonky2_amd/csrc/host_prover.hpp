// host_prover.hpp -- the HOST-POINTER layer of libp2hot: what a patched plonky2 crate calls from the prover's main thread
// with ordinary Vec<F> buffers (include/p2hot.h, "prover session" section).  Included at the end of p2hot.hip (one TU).
//
// Reference call sites this layer stands behind:
//   PolynomialBatch::from_values / from_coeffs   plonky2/src/fri/oracle.rs:57-112      p2hot_commit, p2hot_commit_cols
//   MerkleTree::get / ::prove                      hash/merkle_tree.rs:227, :231-237     p2hot_batch_rows, p2hot_batch_paths
//   OpeningSet::new                                plonk/proof.rs:314-327                p2hot_eval_openings
//   PolynomialBatch::prove_openings + fri_proof    fri/oracle.rs:176-237, fri/prover.rs:24-82, :204-258   p2hot_prove_openings
//   all_wires_permutation_partial_products         plonk/prover.rs:356-449               p2hot_partial_products
//   quotient coset_ifft + chunks                   plonk/prover.rs:274-289, :810-815     p2hot_quotient_chunks
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
extern "C" int p2hot_commit_many_dev(p2hot_ctx *ctx, uint64_t *d_cols, size_t M, size_t W, unsigned log_n, unsigned rate_bits,
                                     unsigned cap_height, int is_values, uint64_t *d_lde, uint64_t *d_digests, uint64_t *d_cap) {
    if (!ctx) return P2HOT_EINVAL;
    DeviceGuard dev_guard_(ctx);
    P2_TRY(check_log(ctx, log_n + rate_bits, "commit_many"));
    if (M == 0) return P2HOT_OK;
    if (W == 0) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: no polynomials (the reference panics on polynomials[0], fri/oracle.rs:90)");
    if (M & (M - 1)) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: the number of proofs (%zu) must be a power of two", M);
    unsigned lm = 0;
    while (((size_t)1 << lm) < M) ++lm;
    const unsigned log_N = log_n + rate_bits;
    if (cap_height > log_N) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: cap_height %u > log2(N) %u (merkle_tree.rs:195-200)", cap_height, log_N);
    if (!d_cols || !d_lde || !d_cap || (p2hot_num_digests(log_N, cap_height) && !d_digests)) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: null buffer");
    if (W * M > 65535) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: W * M = %zu polynomials exceed one launch (65535)", W * M);
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
    if (W == 0) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: no polynomials (the reference panics on polynomials[0], fri/oracle.rs:90)");
    if (M & (M - 1)) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: the number of proofs (%zu) must be a power of two", M);
    if (!cols) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: null column table");
    for (size_t i = 0; i < M * W; ++i)
        if (!cols[i]) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: column %zu of proof %zu is null", i % W, i / W);
    const unsigned log_N = log_n + rate_bits;
    if (cap_height > log_N) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: cap_height %u > log2(N) %u (merkle_tree.rs:195-200)", cap_height, log_N);
    const size_t n = (size_t)1 << log_n, N = n << rate_bits, nd = p2hot_num_digests(log_N, cap_height), cap_words = (size_t)4 << cap_height;
    PoolBuf d_co(ctx), d_lde(ctx), d_dig(ctx), d_cap(ctx);
    P2_TRY(pool_alloc(ctx, W * M * n * 8, &d_co.p));
    P2_TRY(pool_alloc(ctx, W * M * N * 8, &d_lde.p));
    P2_TRY(pool_alloc(ctx, (nd ? nd : 1) * M * 32, &d_dig.p));
    P2_TRY(pool_alloc(ctx, cap_words * M * 8, &d_cap.p));
    auto body = [&]() -> int {
        // interleave on the way in: column e of proof m lands in slot e * M + m (one staged copy for short columns)
        std::vector<const uint64_t *> order(W * M);
        for (size_t e = 0; e < W; ++e)
            for (size_t m = 0; m < M; ++m) order[e * M + m] = cols[m * W + e];
        P2_TRY(h2d_columns(ctx, d_co.u(), order.data(), W * M, n * 8, 0, W * M * n * 8, ctx->stream));
        P2_TRY(p2hot_commit_many_dev(ctx, d_co.u(), M, W, log_n, rate_bits, cap_height, is_values, d_lde.u(), d_dig.u(), d_cap.u()));
        if (coeffs_out)  // [M][W][n] <- [W][M][n]: one strided copy per proof
            for (size_t m = 0; m < M; ++m)
                P2_TRY(d2h_2d(ctx, coeffs_out + m * W * n, n * 8, d_co.u() + m * n, M * n * 8, n * 8, W));
        if (digests_out && nd) P2_TRY(d2h(ctx, digests_out, d_dig.p, nd * M * 32));
        if (caps_out) P2_TRY(d2h(ctx, caps_out, d_cap.p, cap_words * M * 8));
        return P2HOT_OK;
    };
    int rc = sync_checked(ctx, body(), "commit_many");
    if (rc == P2HOT_OK && handles_out) {
        SharedBlocks *sh = new SharedBlocks;
        sh->refs = (int)M;
        sh->lde = d_lde.p;
        sh->dig = d_dig.p;
        sh->coef = d_co.p;
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
    }
    return rc;
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

static int eval_openings_core(p2hot_ctx *ctx, const std::vector<OracleView> &views, unsigned log_n, const uint64_t *points, size_t n_points,
                              uint64_t *out) {
    std::vector<const u64 *> ptrs;
    for (auto &v : views)
        for (size_t j = 0; j < v.W; ++j) ptrs.push_back(v.d_coef + j * v.col_coef(log_n));
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

// ------------------------------------------------------------------ permutation argument (plonk/prover.rs:356-449)
extern "C" int p2hot_partial_products(p2hot_ctx *ctx, const p2hot_cols *wires, size_t wires_first_col, const p2hot_cols *sigmas,
                                      size_t sigmas_first_col, const uint64_t *k_is, unsigned num_routed, unsigned degree,
                                      const uint64_t *betas, const uint64_t *gammas, unsigned num_challenges, uint64_t *out_host,
                                      p2hot_cols **out_cols) {
    P2_ENTER(ctx);
    if (out_cols) *out_cols = nullptr;
    if (!wires || !sigmas || wires->ctx != ctx || sigmas->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "partial_products: null or foreign column set");
    if (wires->log_n != sigmas->log_n) P2_FAIL(ctx, P2HOT_EINVAL, "partial_products: wires and sigmas have different lengths");
    if (wires_first_col > wires->W || num_routed > wires->W - wires_first_col || sigmas_first_col > sigmas->W ||
        num_routed > sigmas->W - sigmas_first_col)
        P2_FAIL(ctx, P2HOT_EINVAL, "partial_products: %u routed columns do not fit the column sets", num_routed);
    // prover.rs:215-218: "When the number of routed wires is smaller that the degree, we should change the logic"
    if (degree < 2 || !(degree < num_routed)) P2_FAIL(ctx, P2HOT_EINVAL, "partial_products: need 2 <= degree < num_routed");
    const unsigned log_n = wires->log_n;
    const size_t n = (size_t)1 << log_n;
    const unsigned num_prods = (num_routed + degree - 1) / degree - 1;
    const size_t rows = (size_t)num_challenges * (num_prods + 1);
    PoolBuf d_out(ctx);
    P2_TRY(pool_alloc(ctx, (rows ? rows : 1) * n * 8, &d_out.p));
    auto body = [&]() -> int {
        P2_TRY(p2hot_partial_products_dev(ctx, wires->d + wires_first_col * n, n, sigmas->d + sigmas_first_col * n, n, k_is, num_routed,
                                          log_n, degree, betas, gammas, num_challenges, d_out.u(), n));
        if (out_host && rows) P2_HIP(ctx, hipMemcpyAsync(out_host, d_out.p, rows * n * 8, hipMemcpyDeviceToHost, ctx->stream));
        return P2HOT_OK;
    };
    int rc = sync_checked(ctx, body(), "partial_products");
    if (rc == P2HOT_OK && out_cols) {
        *out_cols = new p2hot_cols{ctx, d_out.u(), rows, log_n, true};
        d_out.p = nullptr;
    }
    return rc;
}

// ------------------------------------------------------------------ quotient polynomials -> chunks (plonk/prover.rs:274-289, :810-815)
// the tail both quotient entry points share: d_work holds num_challenges polynomials' VALUES on g*H of size m = n << qbits
// (natural order, one flag word behind them); coset_ifft, trim_to_len with its divisibility check, chunks of n
static int quotient_chunks_core(p2hot_ctx *ctx, PoolBuf &d_work, unsigned num_challenges, unsigned degree_bits, unsigned qbits,
                                unsigned quotient_degree_factor, const char *what, p2hot_cols **chunks_out) {
    const size_t n = (size_t)1 << degree_bits, m = n << qbits, keep = n * quotient_degree_factor;
    PoolBuf d_chunks(ctx);
    // (the caller's kernel or uploads into d_work may still be in flight: every early return synchronises before the PoolBufs go back)
    if (int rc0 = pool_alloc(ctx, (num_challenges ? (size_t)num_challenges * quotient_degree_factor : 1) * n * 8, &d_chunks.p))
        return sync_checked(ctx, rc0, what);
    unsigned nonzero = 0;
    auto body = [&]() -> int {
        // values.coset_ifft(F::coset_shift()) (prover.rs:810-814)
        P2_TRY(p2hot_coset_ifft_dev(ctx, d_work.u(), num_challenges, m, degree_bits + qbits, gl::COSET_SHIFT));
        // trim_to_len(quotient_degree_factor * n) (polynomial/mod.rs:164-178) with its divisibility check, then
        // chunks(degree) (mod.rs:136-142): the kept prefix of polynomial c is chunks c*qdf .. (c+1)*qdf-1
        unsigned *flag = (unsigned *)(d_work.u() + (size_t)num_challenges * m);
        P2_HIP(ctx, hipMemsetAsync(flag, 0, 8, ctx->stream));
        for (unsigned c = 0; c < num_challenges; ++c) {
            if (keep < m) {
                P2HOT_LAUNCH(plonk::any_nonzero_kernel, dim3(cdiv(m - keep, 256)), dim3(256), 0, ctx->stream,
                             (const u64 *)(d_work.u() + c * m + keep), m - keep, flag);
                P2_LAUNCH_CHECK(ctx);
            }
            P2_HIP(ctx, hipMemcpyAsync(d_chunks.u() + (size_t)c * keep, d_work.u() + c * m, keep * 8, hipMemcpyDeviceToDevice, ctx->stream));
        }
        if (num_challenges) {
            P2HOT_LAUNCH(ntt::canon_kernel, dim3(cdiv((size_t)num_challenges * keep, 256)), dim3(256), 0, ctx->stream, d_chunks.u(),
                         (size_t)num_challenges * keep);
            P2_LAUNCH_CHECK(ctx);
        }
        P2_HIP(ctx, hipMemcpyAsync(&nonzero, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
        return P2HOT_OK;
    };
    int rc = sync_checked(ctx, body(), what);
    if (rc != P2HOT_OK) return rc;
    if (nonzero) P2_FAIL(ctx, P2HOT_EINVAL, "Quotient has failed, the vanishing polynomial is not divisible by Z_H");
    *chunks_out = new p2hot_cols{ctx, d_chunks.u(), (size_t)num_challenges * quotient_degree_factor, degree_bits, true};
    d_chunks.p = nullptr;
    return P2HOT_OK;
}

extern "C" int p2hot_quotient_chunks(p2hot_ctx *ctx, const uint64_t *const *quotient_values, unsigned num_challenges,
                                     unsigned degree_bits, unsigned quotient_degree_factor, p2hot_cols **chunks_out) {
    P2_ENTER(ctx);
    if (!chunks_out) P2_FAIL(ctx, P2HOT_EINVAL, "quotient_chunks: null output");
    *chunks_out = nullptr;
    if (quotient_degree_factor == 0 || (num_challenges && !quotient_values)) P2_FAIL(ctx, P2HOT_EINVAL, "quotient_chunks: bad arguments");
    unsigned qbits = 0;
    while ((1u << qbits) < quotient_degree_factor) ++qbits;  // log2_ceil (circuit_data.rs quotient_degree_bits)
    P2_TRY(check_log(ctx, degree_bits + qbits, "quotient_chunks"));
    const size_t n = (size_t)1 << degree_bits, m = n << qbits;
    for (unsigned c = 0; c < num_challenges; ++c)  // every argument is checked before the first copy is queued
        if (!quotient_values[c]) P2_FAIL(ctx, P2HOT_EINVAL, "quotient_chunks: polynomial %u is null", c);
    PoolBuf d_work(ctx);
    P2_TRY(pool_alloc(ctx, (num_challenges ? num_challenges : 1) * m * 8 + 8, &d_work.p));
    auto upload = [&]() -> int {
        for (unsigned c = 0; c < num_challenges; ++c)
            P2_HIP(ctx, hipMemcpyAsync(d_work.u() + c * m, quotient_values[c], m * 8, hipMemcpyHostToDevice, ctx->stream));
        return P2HOT_OK;
    };
    if (int rc0 = upload()) return sync_checked(ctx, rc0, "quotient_chunks");  // earlier copies into d_work are drained before it goes back
    return quotient_chunks_core(ctx, d_work, num_challenges, degree_bits, qbits, quotient_degree_factor, "quotient_chunks", chunks_out);
}

// ------------------------------------------------------------------ the standard gates' constraints (gates.hpp; include/p2hot.h)
// every check of a gate set, before anything is enqueued; *max_constraints = the longest constraint list (the alpha-power table's length)
static int gates_validate(p2hot_ctx *ctx, const p2hot_gate_set *gs, const p2hot_batch *wires, const p2hot_batch *constants_sigmas,
                          size_t sigmas_first_col, unsigned quotient_degree_factor, const char *what, unsigned *max_constraints) {
    *max_constraints = 1;
    if (!gs) P2_FAIL(ctx, P2HOT_EINVAL, "%s: null gate set", what);
    if (gs->num_gates && !gs->gates) P2_FAIL(ctx, P2HOT_EINVAL, "%s: %u gates but a null descriptor array", what, gs->num_gates);
    if (sigmas_first_col > constants_sigmas->W) P2_FAIL(ctx, P2HOT_EINVAL, "%s: sigmas_first_col beyond the constants_sigmas commitment", what);
    for (unsigned k = 0; k < gs->num_gates; ++k) {
        const p2hot_gate &g = gs->gates[k];
        if (g.kind > P2HOT_GATE_POSEIDON && (g.kind < P2HOT_GATE_POSEIDON_MDS || g.kind > P2HOT_GATE_COSET_INTERPOLATION))
            P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "%s: gate %u has the unknown kind %u", what, k, g.kind);
        if (g.row < g.group_first || g.row >= g.group_end) P2_FAIL(ctx, P2HOT_EINVAL, "%s: gate %u: row %u outside its group [%u, %u)", what, k, g.row, g.group_first, g.group_end);
        if (g.group_end - g.group_first > 256) P2_FAIL(ctx, P2HOT_EINVAL, "%s: gate %u: a selector group of %u gates (at most 256)", what, k, g.group_end - g.group_first);
        if (g.selector_index >= gs->num_selectors) P2_FAIL(ctx, P2HOT_EINVAL, "%s: gate %u: selector %u of %u", what, k, g.selector_index, gs->num_selectors);
        if (g.kind == P2HOT_GATE_BASE_SUM && (g.param1 < 2 || g.param0 > 63)) P2_FAIL(ctx, P2HOT_EINVAL, "%s: gate %u: BaseSum base %u, %u limbs (B >= 2, at most 63 limbs)", what, k, g.param1, g.param0);
        // the range constraint has degree B and the kernel takes B - 1 products per limb: a circuit whose quotient degree factor is
        // below B cannot hold the gate (gates/selectors.rs:101-160: group size + degree <= factor + 1)
        if (g.kind == P2HOT_GATE_BASE_SUM && g.param1 > quotient_degree_factor)
            P2_FAIL(ctx, P2HOT_EINVAL, "%s: gate %u: BaseSum base %u above the quotient degree factor %u", what, k, g.param1, quotient_degree_factor);
        if (g.param0 > (1u << 24)) P2_FAIL(ctx, P2HOT_EINVAL, "%s: gate %u: parameter %u", what, k, g.param0);
        // the recursion kinds (gates_recursion.hpp): parameter ranges, then the degree against the factor for the reason BaseSum's base
        // is bounded -- a circuit whose factor is below the gate's degree cannot hold it, and the bounds keep the kernel's loops short
        const unsigned qdf = quotient_degree_factor;
        switch (g.kind) {
            case P2HOT_GATE_REDUCING:
            case P2HOT_GATE_REDUCING_EXT: {
                const char *name = g.kind == P2HOT_GATE_REDUCING ? "Reducing" : "ReducingExtension";
                if (g.param0 == 0) P2_FAIL(ctx, P2HOT_EINVAL, "%s: gate %u: %s with 0 coefficients", what, k, name);
                if (qdf < 2) P2_FAIL(ctx, P2HOT_EINVAL, "%s: gate %u: %s degree 2 above the quotient degree factor %u", what, k, name, qdf);
                break;
            }
            case P2HOT_GATE_EXPONENTIATION:
                if (g.param0 == 0) P2_FAIL(ctx, P2HOT_EINVAL, "%s: gate %u: Exponentiation with 0 power bits", what, k);
                if (qdf < 4) P2_FAIL(ctx, P2HOT_EINVAL, "%s: gate %u: Exponentiation degree 4 above the quotient degree factor %u", what, k, qdf);
                break;
            case P2HOT_GATE_RANDOM_ACCESS: {
                const unsigned bits = gates::ra_bits(g), extra = gates::ra_extra(g);
                if (g.param0 == 0) P2_FAIL(ctx, P2HOT_EINVAL, "%s: gate %u: RandomAccess with 0 copies", what, k);
                if (bits < 1 || bits > gates::MAX_ACCESS_BITS) P2_FAIL(ctx, P2HOT_EINVAL, "%s: gate %u: RandomAccess bits %u (1..%u)", what, k, bits, gates::MAX_ACCESS_BITS);
                if (extra > (1u << 16)) P2_FAIL(ctx, P2HOT_EINVAL, "%s: gate %u: RandomAccess with %u extra constants", what, k, extra);
                if (bits + 1 > qdf)
                    P2_FAIL(ctx, P2HOT_EINVAL, "%s: gate %u: RandomAccess bits %u: degree %u above the quotient degree factor %u", what, k, bits, bits + 1, qdf);
                break;
            }
            case P2HOT_GATE_COSET_INTERPOLATION:
                if (g.param0 < 1 || g.param0 > gates::MAX_SUBGROUP_BITS)
                    P2_FAIL(ctx, P2HOT_EINVAL, "%s: gate %u: CosetInterpolation subgroup_bits %u (1..%u)", what, k, g.param0, gates::MAX_SUBGROUP_BITS);
                if (g.param1 < 2 || g.param1 > (1u << g.param0))
                    P2_FAIL(ctx, P2HOT_EINVAL, "%s: gate %u: CosetInterpolation degree %u over %u points (2..%u)", what, k, g.param1, 1u << g.param0, 1u << g.param0);
                if (g.param1 > qdf)
                    P2_FAIL(ctx, P2HOT_EINVAL, "%s: gate %u: CosetInterpolation degree %u above the quotient degree factor %u", what, k, g.param1, qdf);
                break;
            default: break;
        }
        unsigned nw, nk, ncons;
        gates::shape(g, nw, nk, ncons);
        if (nw > wires->W) P2_FAIL(ctx, P2HOT_EINVAL, "%s: gate %u reads %u wires of %zu", what, k, nw, wires->W);
        if ((size_t)gs->num_selectors + gs->num_lookup_selectors + nk > sigmas_first_col)
            P2_FAIL(ctx, P2HOT_EINVAL, "%s: gate %u: %u selectors, %u lookup selectors and %u constants reach past sigmas_first_col = %zu", what, k,
                    gs->num_selectors, gs->num_lookup_selectors, nk, sigmas_first_col);
        if (ncons > *max_constraints) *max_constraints = ncons;
    }
    return P2HOT_OK;
}

// apow HOST [nc][stride]: alpha_a^j, canonical
static void gates_alpha_powers(u64 *apow, const uint64_t *alphas, unsigned nc, unsigned stride) {
    for (unsigned a = 0; a < nc; ++a) {
        u64 pw = 1;
        for (unsigned j = 0; j < stride; ++j, pw = gl::mul(pw, alphas[a])) apow[(size_t)a * stride + j] = gl::canon(pw);
    }
}

// the launches: the cheap kinds MAX_CHEAP descriptors at a time, the recursion kinds the same way, then one launch per PoseidonMdsGate
// and per PoseidonGate; all add into d_out [nc][1 << log_nq].  d_many (p2hot_quotient_polys_gates_many): the M-form kernels, one grid
// row per proof, with d_apow [M][nc][apow_stride], d_out [M][nc][1 << log_nq] and the wires and public-inputs hash of proof y in d_many[y]
#define P2_GATES_LAUNCH(name, args)                                                                                     \
    do {                                                                                                                \
        if (d_many) {                                                                                                   \
            switch (nc) {                                                                                               \
                case 1: P2HOT_LAUNCH((gates::name##_many_kernel<1>), grid, block, 0, ctx->stream, args, d_many); break;  \
                case 2: P2HOT_LAUNCH((gates::name##_many_kernel<2>), grid, block, 0, ctx->stream, args, d_many); break;  \
                case 3: P2HOT_LAUNCH((gates::name##_many_kernel<3>), grid, block, 0, ctx->stream, args, d_many); break;  \
                default: P2HOT_LAUNCH((gates::name##_many_kernel<4>), grid, block, 0, ctx->stream, args, d_many); break; \
            }                                                                                                           \
        } else {                                                                                                        \
            switch (nc) {                                                                                               \
                case 1: P2HOT_LAUNCH((gates::name##_kernel<1>), grid, block, 0, ctx->stream, args); break;               \
                case 2: P2HOT_LAUNCH((gates::name##_kernel<2>), grid, block, 0, ctx->stream, args); break;               \
                case 3: P2HOT_LAUNCH((gates::name##_kernel<3>), grid, block, 0, ctx->stream, args); break;               \
                default: P2HOT_LAUNCH((gates::name##_kernel<4>), grid, block, 0, ctx->stream, args); break;              \
            }                                                                                                           \
        }                                                                                                               \
    } while (0)
static int gates_launch(p2hot_ctx *ctx, const p2hot_gate_set *gs, const p2hot_batch *wires, const p2hot_batch *constants_sigmas,
                        const u64 *d_apow, unsigned apow_stride, u64 *d_out, unsigned log_nq, unsigned nc,
                        const gates::ManyGate *d_many = nullptr, size_t M = 1) {
    const size_t m = (size_t)1 << log_nq;
    const dim3 grid(cdiv(m, 256), (unsigned)M), block(256);
    gates::Args a{};
    a.wires = wires->d_lde, a.wires_stride = wires->col_stride_lde();
    a.consts = constants_sigmas->d_lde, a.consts_stride = constants_sigmas->col_stride_lde();
    a.apow = d_apow, a.apow_stride = apow_stride, a.out = d_out, a.log_nq = log_nq;
    a.num_selectors = gs->num_selectors, a.consts_first = gs->num_selectors + gs->num_lookup_selectors;
    for (unsigned k = 0; k < 4; ++k) a.pih[k] = gl::canon(gs->public_inputs_hash[k]);
    auto flush = [&]() -> int {
        if (!a.num_gates) return P2HOT_OK;
        ProfScope prof(ctx, "gates_cheap");
        P2_GATES_LAUNCH(cheap_gates, a);
        P2_LAUNCH_CHECK(ctx);
        a.num_gates = 0;
        return P2HOT_OK;
    };
    for (unsigned k = 0; k < gs->num_gates; ++k) {
        const p2hot_gate &g = gs->gates[k];
        if (g.kind == P2HOT_GATE_NOOP || g.kind >= P2HOT_GATE_POSEIDON) continue;  // (the recursion kinds have launches of their own below)
        a.gates[a.num_gates++] = g;
        if (a.num_gates == gates::MAX_CHEAP) P2_TRY(flush());
    }
    P2_TRY(flush());
    // the recursion kinds: the descriptor loop of gates_recursion.hpp, the same Args plus CosetInterpolation's domain and 1 / N
    {
        gates::RecursionArgs ra{};
        static_cast<gates::Args &>(ra) = a;
        ra.num_gates = 0;
        const u64 w32 = gl::root_of_unity(gates::MAX_SUBGROUP_BITS);
        u64 x = 1;
        for (unsigned t = 0; t < (1u << gates::MAX_SUBGROUP_BITS); ++t, x = gl::mul(x, w32)) ra.dom[t] = gl::canon(x);
        for (unsigned b = 0; b <= gates::MAX_SUBGROUP_BITS; ++b) ra.ninv[b] = gl::canon(gl::inv((u64)1 << b));
        auto flush_rec = [&]() -> int {
            if (!ra.num_gates) return P2HOT_OK;
            ProfScope prof(ctx, "gates_recursion");
            P2_GATES_LAUNCH(recursion_gates, ra);
            P2_LAUNCH_CHECK(ctx);
            ra.num_gates = 0;
            return P2HOT_OK;
        };
        for (unsigned k = 0; k < gs->num_gates; ++k) {
            const p2hot_gate &g = gs->gates[k];
            if (g.kind < P2HOT_GATE_REDUCING || g.kind > P2HOT_GATE_COSET_INTERPOLATION) continue;
            ra.gates[ra.num_gates++] = g;
            if (ra.num_gates == gates::MAX_CHEAP) P2_TRY(flush_rec());
        }
        P2_TRY(flush_rec());
    }
    for (unsigned k = 0; k < gs->num_gates; ++k) {
        if (gs->gates[k].kind != P2HOT_GATE_POSEIDON_MDS) continue;
        gates::PoseidonArgs pa{};
        pa.wires = a.wires, pa.wires_stride = a.wires_stride, pa.consts = a.consts, pa.consts_stride = a.consts_stride;
        pa.apow = d_apow, pa.apow_stride = apow_stride, pa.out = d_out, pa.log_nq = log_nq, pa.num_selectors = gs->num_selectors;
        pa.gate = gs->gates[k];
        ProfScope prof(ctx, "gates_poseidon_mds");
        P2_GATES_LAUNCH(mds_gate, pa);
        P2_LAUNCH_CHECK(ctx);
    }
    for (unsigned k = 0; k < gs->num_gates; ++k) {
        if (gs->gates[k].kind != P2HOT_GATE_POSEIDON) continue;
        gates::PoseidonArgs pa{};
        pa.wires = a.wires, pa.wires_stride = a.wires_stride, pa.consts = a.consts, pa.consts_stride = a.consts_stride;
        pa.apow = d_apow, pa.apow_stride = apow_stride, pa.out = d_out, pa.log_nq = log_nq, pa.num_selectors = gs->num_selectors;
        pa.gate = gs->gates[k];
        ProfScope prof(ctx, "gates_poseidon");
        P2_GATES_LAUNCH(poseidon_gate, pa);
        P2_LAUNCH_CHECK(ctx);
    }
    return P2HOT_OK;
}

// ------------------------------------------------------------------ gate programs (gate_program.hpp; include/p2hot.h)
// the checked programs of one call as one device block: public_inputs_hash, the constants, the headers, then the instructions
struct GateProgPlan {
    std::vector<u64> blob;  // host image of the device block (outlives the asynchronous copy)
    size_t n_consts = 0, n_gates = 0, n_insns = 0;
    unsigned num_temps = 0;
    bool empty() const { return n_gates == 0; }
};

// every check of the programs, before anything is enqueued (include/p2hot.h lists them); `gs` has passed gates_validate.
// *max_constraints grows to the longest constraint list among the programs (the alpha-power table's length)
static int gate_programs_validate(p2hot_ctx *ctx, const p2hot_gate_program *programs, unsigned num_programs, const p2hot_gate_set *gs,
                                  const p2hot_batch *wires, size_t sigmas_first_col, unsigned quotient_degree_factor, const char *what,
                                  unsigned *max_constraints, GateProgPlan *pl) {
    if (num_programs == 0) return P2HOT_OK;
    if (!programs) P2_FAIL(ctx, P2HOT_EINVAL, "%s: %u gate programs but a null program array", what, num_programs);
    const size_t consts_first = (size_t)gs->num_selectors + gs->num_lookup_selectors;
    const u32 unwritten = ~0u, sat = 1u << 20;
    std::vector<p2hot_air_insn> insns;
    std::vector<u64> constants;
    std::vector<gateprog::Header> headers(num_programs);
    std::set<u32> rows;
    for (unsigned k = 0; k < gs->num_gates; ++k) rows.insert(gs->gates[k].row);
    for (unsigned p = 0; p < num_programs; ++p) {
        const p2hot_gate_program &g = programs[p];
        const p2hot_air_program &pr = g.program;
        if ((pr.num_insns && !pr.insns) || (pr.num_constants && !pr.constants))
            P2_FAIL(ctx, P2HOT_EINVAL, "%s: program %u: a program array is null but its count is not", what, p);
        if (g.row < g.group_first || g.row >= g.group_end) P2_FAIL(ctx, P2HOT_EINVAL, "%s: program %u: row %u outside its group [%u, %u)", what, p, g.row, g.group_first, g.group_end);
        if (g.group_end - g.group_first > 256) P2_FAIL(ctx, P2HOT_EINVAL, "%s: program %u: a selector group of %u gates (at most 256)", what, p, g.group_end - g.group_first);
        if (g.selector_index >= gs->num_selectors) P2_FAIL(ctx, P2HOT_EINVAL, "%s: program %u: selector %u of %u", what, p, g.selector_index, gs->num_selectors);
        if (consts_first > sigmas_first_col)  // (the selector column itself must lie in front of the sigmas)
            P2_FAIL(ctx, P2HOT_EINVAL, "%s: program %u: %u selectors and %u lookup selectors reach past sigmas_first_col = %zu", what, p, gs->num_selectors,
                    gs->num_lookup_selectors, sigmas_first_col);
        if (!rows.insert(g.row).second)
            P2_FAIL(ctx, P2HOT_EINVAL, "%s: program %u: row %u is already a gate of this call (a descriptor of the set or an earlier program)", what, p, g.row);
        if (pr.num_publics > 4) P2_FAIL(ctx, P2HOT_EINVAL, "%s: program %u names %u words of a public_inputs_hash of 4", what, p, pr.num_publics);
        if (pr.num_temps > air::MAX_TEMPS)
            P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "%s: program %u uses %u temp slots (p2hot_air_max_temps() = %u)", what, p, pr.num_temps, air::MAX_TEMPS);
        // the filter's degree (gate.rs:326-333) on top of every constraint's; max_degree = factor + 1 (gates/selectors.rs:101-160)
        const u32 filter_degree = g.group_end - g.group_first - 1 + (gs->num_selectors > 1 ? 1 : 0), max_degree = quotient_degree_factor + 1;
        std::vector<u32> tdeg(pr.num_temps, unwritten);
        unsigned ncons = 0;
        for (u32 k = 0; k < pr.num_insns; ++k) {
            p2hot_air_insn in = pr.insns[k];
            if (in.op > P2HOT_AIR_CONSTRAINT_LAST_ROW) P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "%s: program %u: instruction %u: unknown op %u", what, p, k, in.op);
            if (in.op > P2HOT_AIR_CONSTRAINT)
                P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "%s: program %u: instruction %u: op %u is a STARK consumer's filtered constraint, not a gate's", what, p, k, in.op);
            const bool arith = in.op <= P2HOT_AIR_MUL;
            u32 deg[2] = {0, 0};
            for (int s = 0; s < (arith ? 2 : 1); ++s) {
                u32 &o = s ? in.b : in.a;
                const u32 kind = o >> air::KIND_SHIFT, idx = o & air::INDEX_MASK;
                const char side = s ? 'b' : 'a';
                switch (kind) {
                    case P2HOT_AIR_LOCAL:
                        if (idx >= wires->W) P2_FAIL(ctx, P2HOT_EINVAL, "%s: program %u: instruction %u: operand %c reads wire %u of %zu", what, p, k, side, idx, wires->W);
                        deg[s] = 1;
                        break;
                    case P2HOT_AIR_GATE_CONST:
                        if (consts_first + idx >= sigmas_first_col)
                            P2_FAIL(ctx, P2HOT_EINVAL, "%s: program %u: instruction %u: operand %c reads gate constant %u: %u selectors, %u lookup selectors and it reach sigmas_first_col = %zu",
                                    what, p, k, side, idx, gs->num_selectors, gs->num_lookup_selectors, sigmas_first_col);
                        deg[s] = 1;
                        break;
                    case P2HOT_AIR_NEXT:
                        P2_FAIL(ctx, P2HOT_EINVAL, "%s: program %u: instruction %u: operand %c reads the next row, which a gate does not see", what, p, k, side);
                    case P2HOT_AIR_PUBLIC:
                        if (idx >= pr.num_publics) P2_FAIL(ctx, P2HOT_EINVAL, "%s: program %u: instruction %u: operand %c reads hash word %u of %u", what, p, k, side, idx, pr.num_publics);
                        break;
                    case P2HOT_AIR_CONST:
                        if (idx >= pr.num_constants) P2_FAIL(ctx, P2HOT_EINVAL, "%s: program %u: instruction %u: operand %c reads constant %u of %u", what, p, k, side, idx, pr.num_constants);
                        o = P2HOT_AIR_OPERAND(P2HOT_AIR_CONST, constants.size() + idx);  // rebased into the call's one constant array
                        break;
                    case P2HOT_AIR_TEMP:
                        if (idx >= pr.num_temps) P2_FAIL(ctx, P2HOT_EINVAL, "%s: program %u: instruction %u: operand %c reads temp %u of %u", what, p, k, side, idx, pr.num_temps);
                        if (tdeg[idx] == unwritten) P2_FAIL(ctx, P2HOT_EINVAL, "%s: program %u: instruction %u: operand %c reads temp %u before any instruction wrote it", what, p, k, side, idx);
                        deg[s] = tdeg[idx];
                        break;
                    default:
                        P2_FAIL(ctx, P2HOT_EINVAL, "%s: program %u: instruction %u: operand %c has the unknown kind %u", what, p, k, side, kind);
                }
            }
            if (arith) {
                if (in.dst >= pr.num_temps) P2_FAIL(ctx, P2HOT_EINVAL, "%s: program %u: instruction %u writes temp %u of %u", what, p, k, in.dst, pr.num_temps);
                tdeg[in.dst] = std::min(sat, in.op == P2HOT_AIR_MUL ? deg[0] + deg[1] : std::max(deg[0], deg[1]));
            } else {
                if (deg[0] + filter_degree > max_degree)
                    P2_FAIL(ctx, P2HOT_EINVAL, "%s: program %u: instruction %u: a constraint of degree %u under a filter of degree %u, above quotient_degree_factor + 1 = %u",
                            what, p, k, deg[0], filter_degree, max_degree);
                ++ncons;
            }
            insns.push_back(in);
        }
        if (constants.size() + pr.num_constants > air::INDEX_MASK) P2_FAIL(ctx, P2HOT_EINVAL, "%s: program %u: the programs' constants do not fit an operand index", what, p);
        gateprog::Header &h = headers[p];
        h.gate = p2hot_gate{0, g.row, g.selector_index, g.group_first, g.group_end, 0, 0};
        h.insn_first = (u32)(insns.size() - pr.num_insns), h.insn_end = (u32)insns.size(), h.pad = 0;
        for (u32 k = 0; k < pr.num_constants; ++k) constants.push_back(gl::canon(pr.constants[k]));
        pl->num_temps = std::max(pl->num_temps, pr.num_temps);
        if (ncons > *max_constraints) *max_constraints = ncons;
    }
    pl->n_consts = constants.size(), pl->n_gates = num_programs, pl->n_insns = insns.size();
    pl->blob.assign(4 + pl->n_consts + 5 * pl->n_gates + 2 * pl->n_insns + 1, 0);
    for (unsigned k = 0; k < 4; ++k) pl->blob[k] = gl::canon(gs->public_inputs_hash[k]);
    std::copy(constants.begin(), constants.end(), pl->blob.begin() + 4);
    memcpy(pl->blob.data() + 4 + pl->n_consts, headers.data(), headers.size() * sizeof(gateprog::Header));
    if (!insns.empty()) memcpy(pl->blob.data() + 4 + pl->n_consts + 5 * pl->n_gates, insns.data(), insns.size() * sizeof(p2hot_air_insn));
    return P2HOT_OK;
}

// uploads the block and evaluates every program gate in one launch, adding into d_out [nc][1 << log_nq] like the gate kernels
static int gate_programs_launch(p2hot_ctx *ctx, const GateProgPlan &pl, PoolBuf &d_blob, const p2hot_gate_set *gs, const p2hot_batch *wires,
                                const p2hot_batch *constants_sigmas, const u64 *d_apow, unsigned apow_stride, u64 *d_out, unsigned log_nq,
                                unsigned nc) {
    if (pl.empty()) return P2HOT_OK;
    P2_HIP(ctx, hipMemcpyAsync(d_blob.p, pl.blob.data(), pl.blob.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    gateprog::Args a{};
    a.pih = d_blob.u(), a.constants = d_blob.u() + 4;
    a.headers = (const gateprog::Header *)(d_blob.u() + 4 + pl.n_consts);
    a.insns = (const p2hot_air_insn *)(d_blob.u() + 4 + pl.n_consts + 5 * pl.n_gates);
    a.wires = wires->d_lde, a.wires_stride = wires->col_stride_lde();
    a.consts = constants_sigmas->d_lde, a.consts_stride = constants_sigmas->col_stride_lde();
    a.apow = d_apow, a.apow_stride = apow_stride, a.out = d_out, a.log_nq = log_nq, a.num_gates = (unsigned)pl.n_gates;
    a.num_selectors = gs->num_selectors, a.consts_first = gs->num_selectors + gs->num_lookup_selectors;
    ProfScope prof(ctx, "gate_programs");
    const size_t shm = (size_t)(pl.num_temps ? pl.num_temps : 1) * gateprog::BLOCK * 8;
    const dim3 grid(cdiv((size_t)1 << log_nq, gateprog::BLOCK)), block(gateprog::BLOCK);
    switch (nc) {
        case 1:
            P2_TRY(lds_opt_in(ctx, reinterpret_cast<const void *>(gateprog::interp_kernel<1>), shm));
            P2HOT_LAUNCH((gateprog::interp_kernel<1>), grid, block, shm, ctx->stream, a);
            break;
        case 2:
            P2_TRY(lds_opt_in(ctx, reinterpret_cast<const void *>(gateprog::interp_kernel<2>), shm));
            P2HOT_LAUNCH((gateprog::interp_kernel<2>), grid, block, shm, ctx->stream, a);
            break;
        case 3:
            P2_TRY(lds_opt_in(ctx, reinterpret_cast<const void *>(gateprog::interp_kernel<3>), shm));
            P2HOT_LAUNCH((gateprog::interp_kernel<3>), grid, block, shm, ctx->stream, a);
            break;
        default:
            P2_TRY(lds_opt_in(ctx, reinterpret_cast<const void *>(gateprog::interp_kernel<4>), shm));
            P2HOT_LAUNCH((gateprog::interp_kernel<4>), grid, block, shm, ctx->stream, a);
            break;
    }
    P2_LAUNCH_CHECK(ctx);
    return P2HOT_OK;
}

// the reduced gate sums on their own (include/p2hot.h): evaluate_gate_constraints_base_batch (plonk/vanishing_poly.rs:702-728) for
// the gates of the set and the program gates, reduced by the powers of every alpha
static int gate_sums_core(p2hot_ctx *ctx, const p2hot_batch *wires, const p2hot_batch *constants_sigmas, size_t sigmas_first_col,
                          const p2hot_gate_set *gates, unsigned quotient_degree_factor, const uint64_t *alphas, unsigned num_challenges,
                          uint64_t *out_host, const p2hot_gate_program *programs, unsigned num_programs) {
    P2_ENTER(ctx);
    if (!wires || !constants_sigmas || !alphas || !out_host) P2_FAIL(ctx, P2HOT_EINVAL, "gate_sums: null argument");
    if (wires->ctx != ctx || constants_sigmas->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "gate_sums: a commitment belongs to another context");
    if (constants_sigmas->log_n != wires->log_n || constants_sigmas->rate_bits != wires->rate_bits)
        P2_FAIL(ctx, P2HOT_EINVAL, "gate_sums: the commitments differ in degree or rate");
    if (num_challenges == 0 || num_challenges > 4) P2_FAIL(ctx, P2HOT_EINVAL, "gate_sums: %u challenges (1..4)", num_challenges);
    if (quotient_degree_factor < 2) P2_FAIL(ctx, P2HOT_EINVAL, "gate_sums: bad quotient degree factor");
    unsigned qbits = 0;
    while ((1u << qbits) < quotient_degree_factor) ++qbits;
    if (qbits > wires->rate_bits) P2_FAIL(ctx, P2HOT_EINVAL, "gate_sums: quotient degree 2^%u above the rate 2^%u (prover.rs:632-636)", qbits, wires->rate_bits);
    unsigned stride = 1;
    P2_TRY(gates_validate(ctx, gates, wires, constants_sigmas, sigmas_first_col, quotient_degree_factor, "gate_sums", &stride));
    GateProgPlan plan;
    P2_TRY(gate_programs_validate(ctx, programs, num_programs, gates, wires, sigmas_first_col, quotient_degree_factor, "gate_sums_programs", &stride, &plan));
    const unsigned log_nq = wires->log_n + qbits;
    const size_t m = (size_t)1 << log_nq;
    PoolBuf d_out(ctx), d_apow(ctx), d_prog(ctx);
    if (!plan.empty()) P2_TRY(pool_alloc(ctx, plan.blob.size() * 8, &d_prog.p));
    P2_TRY(pool_alloc(ctx, (size_t)num_challenges * m * 8, &d_out.p));
    P2_TRY(pool_alloc(ctx, (size_t)num_challenges * stride * 8, &d_apow.p));
    std::vector<u64> apow((size_t)num_challenges * stride);
    gates_alpha_powers(apow.data(), alphas, num_challenges, stride);
    auto body = [&]() -> int {
        P2_HIP(ctx, hipMemcpyAsync(d_apow.p, apow.data(), apow.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        P2_HIP(ctx, hipMemsetAsync(d_out.p, 0, (size_t)num_challenges * m * 8, ctx->stream));
        P2_TRY(gates_launch(ctx, gates, wires, constants_sigmas, d_apow.u(), stride, d_out.u(), log_nq, num_challenges));
        P2_TRY(gate_programs_launch(ctx, plan, d_prog, gates, wires, constants_sigmas, d_apow.u(), stride, d_out.u(), log_nq, num_challenges));
        P2_HIP(ctx, hipMemcpyAsync(out_host, d_out.p, (size_t)num_challenges * m * 8, hipMemcpyDeviceToHost, ctx->stream));
        return P2HOT_OK;
    };
    return sync_checked(ctx, body(), "gate_sums");
}

extern "C" int p2hot_gate_sums(p2hot_ctx *ctx, const p2hot_batch *wires, const p2hot_batch *constants_sigmas, size_t sigmas_first_col,
                               const p2hot_gate_set *gates, unsigned quotient_degree_factor, const uint64_t *alphas, unsigned num_challenges,
                               uint64_t *out_host) {
    return gate_sums_core(ctx, wires, constants_sigmas, sigmas_first_col, gates, quotient_degree_factor, alphas, num_challenges, out_host, nullptr, 0);
}

extern "C" int p2hot_gate_sums_programs(p2hot_ctx *ctx, const p2hot_batch *wires, const p2hot_batch *constants_sigmas, size_t sigmas_first_col,
                                        const p2hot_gate_set *gates, unsigned quotient_degree_factor, const uint64_t *alphas,
                                        unsigned num_challenges, uint64_t *out_host, const p2hot_gate_program *programs, unsigned num_programs) {
    return gate_sums_core(ctx, wires, constants_sigmas, sigmas_first_col, gates, quotient_degree_factor, alphas, num_challenges, out_host, programs,
                          num_programs);
}

// compute_quotient_polys (plonky2/src/plonk/prover.rs:609-815) without its gate evaluation: the permutation argument's vanishing
// terms on the quotient coset (plonk/vanishing_poly.rs:167-330; kernel: plonk::quotient_perm_kernel) from the three commitments'
// device-resident LDE matrices, plus the caller's reduced gate terms, over Z_H; then the same tail as p2hot_quotient_chunks.
// `lk` (p2hot_quotient_polys_lookup): the lookup argument's terms (lookup::lookup_terms_kernel) go between the permutation terms and
// the gate terms; null = p2hot_quotient_polys.  `gs` (p2hot_quotient_polys_gates / _lookup_gates): the set's gates are evaluated on the
// device (gates.hpp) into the gate-sum buffer, on top of the caller's gate_sums, in front of both; null = none
struct LookupQuot {
    unsigned num_lu_slots, num_lut_slots, num_luts;
    size_t selectors_first_col;
    const uint64_t *deltas, *lut_re_poly_evals;
};
static int quotient_polys_core(p2hot_ctx *ctx, const p2hot_batch *wires, const p2hot_batch *constants_sigmas, size_t sigmas_first_col,
                               const p2hot_batch *zs_partial_products, const uint64_t *k_is, unsigned num_routed,
                               unsigned quotient_degree_factor, const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas,
                               unsigned num_challenges, const uint64_t *const *gate_sums, uint64_t *values_out, p2hot_cols **chunks_out,
                               const LookupQuot *lk, const p2hot_gate_set *gs = nullptr, bool with_gates = false,
                               const p2hot_gate_program *programs = nullptr, unsigned num_programs = 0) {
    P2_ENTER(ctx);
    if (chunks_out) *chunks_out = nullptr;
    if (!wires || !constants_sigmas || !zs_partial_products || !k_is || !betas || !gammas || !alphas) P2_FAIL(ctx, P2HOT_EINVAL, "quotient_polys: null argument");
    if (!chunks_out && !values_out) P2_FAIL(ctx, P2HOT_EINVAL, "quotient_polys: nothing asked for");
    const p2hot_batch *bs[3] = {wires, constants_sigmas, zs_partial_products};
    for (const p2hot_batch *b : bs) {
        if (b->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "quotient_polys: a commitment belongs to another context");
        if (b->log_n != wires->log_n || b->rate_bits != wires->rate_bits) P2_FAIL(ctx, P2HOT_EINVAL, "quotient_polys: the commitments differ in degree or rate");
    }
    if (lk && (num_challenges == 0 || num_challenges > 4)) P2_FAIL(ctx, P2HOT_EINVAL, "quotient_polys_lookup: %u challenges (1..4)", num_challenges);
    if (num_challenges == 0 || num_challenges > 4) P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "quotient_polys: %u challenges (1..4 supported; plonky2's configs use 2)", num_challenges);
    if (quotient_degree_factor < 2 || num_routed == 0) P2_FAIL(ctx, P2HOT_EINVAL, "quotient_polys: bad quotient degree factor or no routed wires");
    unsigned qbits = 0;
    while ((1u << qbits) < quotient_degree_factor) ++qbits;
    // "Having constraints of degree higher than the rate is not supported yet." (prover.rs:632-636)
    if (qbits > wires->rate_bits) P2_FAIL(ctx, P2HOT_EINVAL, "quotient_polys: quotient degree 2^%u above the rate 2^%u (prover.rs:632-636)", qbits, wires->rate_bits);
    const unsigned degree_bits = wires->log_n, log_nq = degree_bits + qbits;
    const unsigned num_chunks = (num_routed + quotient_degree_factor - 1) / quotient_degree_factor, num_prods = num_chunks - 1;
    if (wires->W < num_routed || constants_sigmas->W < sigmas_first_col + num_routed || zs_partial_products->W < (size_t)num_challenges * (1 + num_prods))
        P2_FAIL(ctx, P2HOT_EINVAL, "quotient_polys: a commitment is narrower than the permutation argument needs");
    const size_t n = (size_t)1 << degree_bits, m = n << qbits, rate = (size_t)1 << qbits;
    for (unsigned c = 0; c < num_challenges && gate_sums; ++c)
        if (!gate_sums[c]) P2_FAIL(ctx, P2HOT_EINVAL, "quotient_polys: gate_sums[%u] is null", c);
    // the lookup argument (vanishing_poly.rs:515-664): S partial SLDC polynomials + RE per challenge behind the partial products
    unsigned lk_S = 0, lk_Kc = 0;
    if (lk) {
        for (const p2hot_batch *b : bs)
            if (b->hash_n) P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "quotient_polys_lookup: KeccakHash commitments are not supported");
        if (!lk->deltas || (lk->num_luts && !lk->lut_re_poly_evals)) P2_FAIL(ctx, P2HOT_EINVAL, "quotient_polys_lookup: null argument");
        const unsigned lookup_degree = quotient_degree_factor - 1;  // vanishing_poly.rs:526
        if (lk->num_lu_slots == 0 || lk->num_lut_slots == 0) P2_FAIL(ctx, P2HOT_EINVAL, "quotient_polys_lookup: no lookup slots");
        if ((size_t)2 * lk->num_lu_slots > wires->W || (size_t)3 * lk->num_lut_slots > wires->W)
            P2_FAIL(ctx, P2HOT_EINVAL, "quotient_polys_lookup: %u LookupGate / %u LookupTableGate slots do not fit %zu wires", lk->num_lu_slots, lk->num_lut_slots, wires->W);
        lk_S = (lk->num_lu_slots + lookup_degree - 1) / lookup_degree;
        lk_Kc = 4 + lk->num_luts + 2 * lk_S;
        if (zs_partial_products->W != (size_t)num_challenges * (1 + num_prods) + (size_t)num_challenges * (lk_S + 1))
            P2_FAIL(ctx, P2HOT_EINVAL, "quotient_polys_lookup: the Zs batch has %zu polynomials, not nc (1 + %u) + nc (%u + 1)", zs_partial_products->W, num_prods, lk_S);
        if (lk->selectors_first_col > constants_sigmas->W || (size_t)4 + lk->num_luts > constants_sigmas->W - lk->selectors_first_col)
            P2_FAIL(ctx, P2HOT_EINVAL, "quotient_polys_lookup: the lookup selectors do not fit the constants_sigmas commitment");
    }
    unsigned gs_stride = 0;
    GateProgPlan plan;
    if (with_gates) {
        P2_TRY(gates_validate(ctx, gs, wires, constants_sigmas, sigmas_first_col, quotient_degree_factor, "quotient_polys_gates", &gs_stride));
        P2_TRY(gate_programs_validate(ctx, programs, num_programs, gs, wires, sigmas_first_col, quotient_degree_factor, "quotient_polys_gate_programs",
                                      &gs_stride, &plan));
    }
    const size_t n_apow = lk ? (size_t)num_challenges * ((size_t)num_challenges * lk_Kc + 1) : 0, n_evals = lk ? (size_t)num_challenges * lk->num_luts : 0;
    const size_t n_gpow = (size_t)num_challenges * gs_stride;
    PoolBuf d_work(ctx), d_small(ctx), d_gate(ctx), d_prog(ctx);
    if (!plan.empty()) P2_TRY(pool_alloc(ctx, plan.blob.size() * 8, &d_prog.p));
    P2_TRY(pool_alloc(ctx, (size_t)num_challenges * m * 8 + 8, &d_work.p));
    const size_t nbk = (size_t)num_challenges * num_routed;
    P2_TRY(pool_alloc(ctx, (nbk + 2 * rate + n_apow + n_evals + n_gpow) * 8, &d_small.p));
    if (gate_sums || lk || with_gates) P2_TRY(pool_alloc(ctx, (size_t)num_challenges * m * 8, &d_gate.p));
    // ZeroPolyOnCoset::new(degree_bits, qbits) (field/src/zero_poly_coset.rs:21-34) and beta_c * k_j, on the host
    std::vector<u64> small(nbk + 2 * rate + n_apow + n_evals + n_gpow);
    if (with_gates) gates_alpha_powers(small.data() + nbk + 2 * rate + n_apow + n_evals, alphas, num_challenges, gs_stride);
    for (unsigned c = 0; c < num_challenges; ++c)
        for (unsigned j = 0; j < num_routed; ++j) small[(size_t)c * num_routed + j] = gl::canon(gl::mul(betas[c], k_is[j]));
    const size_t num_routed_ = nbk;  // (offset of the Z_H table behind the beta * k table)
    const u64 g_pow_n = gl::pow(gl::COSET_SHIFT, n), v = gl::root_of_unity(qbits);
    for (size_t j = 0; j < rate; ++j) {
        const u64 e = gl::canon(gl::sub(gl::mul(g_pow_n, gl::pow(v, j)), 1));
        if (e == 0) P2_FAIL(ctx, P2HOT_EINVAL, "quotient_polys: Z_H vanishes on the coset");
        small[num_routed_ + j] = e;
        small[num_routed_ + rate + j] = gl::inv(e);
    }
    // 1 / (n (x - 1)) for every point of the quotient coset: sizes only, kept by the context
    const auto inv_key = std::make_tuple(100, log_nq, qbits);
    auto inv_it = ctx->twid_cache.find(inv_key);
    if (inv_it == ctx->twid_cache.end()) {
        u64 *t = nullptr;
        P2_HIP(ctx, hipMalloc((void **)&t, m * 8));
        P2HOT_LAUNCH(plonk::quot_inv_kernel, dim3(cdiv(m, 256)), dim3(256), 0, ctx->stream, t, log_nq, (u64)n % gl::P, ctx->fwd);
        if (hipGetLastError() != hipSuccess) {
            (void)hipFree(t);
            P2_FAIL(ctx, P2HOT_EHIP, "quotient_polys: the L_0 denominator table could not be launched");
        }
        inv_it = ctx->twid_cache.emplace(inv_key, t).first;
    }
    plonk::QuotArgs q{};
    q.wires = wires->d_lde, q.wires_stride = wires->col_stride_lde();
    q.sigmas = constants_sigmas->d_lde + sigmas_first_col * constants_sigmas->col_stride_lde(), q.sigmas_stride = constants_sigmas->col_stride_lde();
    q.zs = zs_partial_products->d_lde, q.zs_stride = zs_partial_products->col_stride_lde();
    q.bk = d_small.u(), q.zh = d_small.u() + nbk, q.inv_nx1 = inv_it->second;
    q.gate_sums = gate_sums || lk || with_gates ? d_gate.u() : nullptr;
    q.out = d_work.u();
    q.num_routed = num_routed, q.degree = quotient_degree_factor, q.num_chunks = num_chunks, q.log_nq = log_nq, q.qbits = qbits;
    const u64 K = (u64)num_challenges + (u64)num_challenges * num_chunks;
    for (unsigned a = 0; a < num_challenges; ++a) {
        q.betas[a] = betas[a], q.gammas[a] = gl::canon(gammas[a]), q.alphas[a] = alphas[a];
        q.alpha_k[a] = gl::pow(alphas[a], K);
        for (unsigned c = 0; c < num_challenges; ++c) q.base[a][c] = gl::pow(alphas[a], (u64)num_challenges + (u64)c * num_chunks);
    }
    q.roots = ctx->fwd;
    lookup::TermArgs lt{};
    if (lk) {
        const unsigned Klu = num_challenges * lk_Kc;
        u64 *apow = small.data() + nbk + 2 * rate, *evals = apow + n_apow;
        for (unsigned a = 0; a < num_challenges; ++a) {
            u64 pw = 1;
            for (unsigned t = 0; t <= Klu; ++t, pw = gl::mul(pw, alphas[a])) apow[(size_t)a * (Klu + 1) + t] = gl::canon(pw);
        }
        for (size_t k = 0; k < n_evals; ++k) evals[k] = gl::canon(lk->lut_re_poly_evals[k]);
        lt.wires = wires->d_lde, lt.wires_stride = wires->col_stride_lde();
        lt.sel = constants_sigmas->d_lde + lk->selectors_first_col * constants_sigmas->col_stride_lde(), lt.sel_stride = constants_sigmas->col_stride_lde();
        lt.lz_stride = zs_partial_products->col_stride_lde();
        lt.lz = zs_partial_products->d_lde + (size_t)num_challenges * (1 + num_prods) * lt.lz_stride;
        lt.apow = d_small.u() + nbk + 2 * rate, lt.lut_evals = lt.apow + n_apow;
        lt.gate_sums = gate_sums || with_gates ? d_gate.u() : nullptr, lt.out = d_gate.u();
        lt.num_lu_slots = lk->num_lu_slots, lt.num_lut_slots = lk->num_lut_slots, lt.lu_degree = quotient_degree_factor - 1;
        lt.S = lk_S, lt.lut_degree = (lk->num_lut_slots + lk_S - 1) / lk_S, lt.num_luts = lk->num_luts, lt.log_nq = log_nq, lt.qbits = qbits;
        for (unsigned c = 0; c < num_challenges; ++c)
            for (unsigned k = 0; k < 4; ++k) lt.deltas[c][k] = gl::canon(lk->deltas[(size_t)c * 4 + k]);
    }
    auto body = [&]() -> int {
        P2_HIP(ctx, hipMemcpyAsync(d_small.p, small.data(), small.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        for (unsigned c = 0; c < num_challenges && gate_sums; ++c)
            P2_HIP(ctx, hipMemcpyAsync(d_gate.u() + (size_t)c * m, gate_sums[c], m * 8, hipMemcpyHostToDevice, ctx->stream));
        if (with_gates) {  // on top of the caller's residual sums (or of zeros)
            if (!gate_sums) P2_HIP(ctx, hipMemsetAsync(d_gate.p, 0, (size_t)num_challenges * m * 8, ctx->stream));
            P2_TRY(gates_launch(ctx, gs, wires, constants_sigmas, d_small.u() + nbk + 2 * rate + n_apow + n_evals, gs_stride, d_gate.u(), log_nq, num_challenges));
            P2_TRY(gate_programs_launch(ctx, plan, d_prog, gs, wires, constants_sigmas, d_small.u() + nbk + 2 * rate + n_apow + n_evals, gs_stride, d_gate.u(),
                                        log_nq, num_challenges));
        }
        if (lk) {
            ProfScope prof(ctx, "quotient_lookup");
            const dim3 grid(cdiv(m, 256)), block(256);
            switch (num_challenges) {
                case 1: P2HOT_LAUNCH((lookup::lookup_terms_kernel<1>), grid, block, 0, ctx->stream, lt); break;
                case 2: P2HOT_LAUNCH((lookup::lookup_terms_kernel<2>), grid, block, 0, ctx->stream, lt); break;
                case 3: P2HOT_LAUNCH((lookup::lookup_terms_kernel<3>), grid, block, 0, ctx->stream, lt); break;
                default: P2HOT_LAUNCH((lookup::lookup_terms_kernel<4>), grid, block, 0, ctx->stream, lt); break;
            }
            P2_LAUNCH_CHECK(ctx);
        }
        ProfScope prof(ctx, "quotient_perm");
        const dim3 grid(cdiv(m, 256)), block(256);
        if (num_challenges == 2 && quotient_degree_factor == 8) {  // every plonky2 config (circuit_data.rs:101-119): the pipelined instantiation
            P2HOT_LAUNCH((plonk::quotient_perm_kernel<2, 8>), grid, block, 0, ctx->stream, q);
        } else {
            switch (num_challenges) {
                case 1: P2HOT_LAUNCH((plonk::quotient_perm_kernel<1, 0>), grid, block, 0, ctx->stream, q); break;
                case 2: P2HOT_LAUNCH((plonk::quotient_perm_kernel<2, 0>), grid, block, 0, ctx->stream, q); break;
                case 3: P2HOT_LAUNCH((plonk::quotient_perm_kernel<3, 0>), grid, block, 0, ctx->stream, q); break;
                default: P2HOT_LAUNCH((plonk::quotient_perm_kernel<4, 0>), grid, block, 0, ctx->stream, q); break;
            }
        }
        P2_LAUNCH_CHECK(ctx);
        if (values_out) P2_HIP(ctx, hipMemcpyAsync(values_out, d_work.p, (size_t)num_challenges * m * 8, hipMemcpyDeviceToHost, ctx->stream));
        return P2HOT_OK;
    };
    int rc = body();
    if (rc != P2HOT_OK || !chunks_out) return sync_checked(ctx, rc, "quotient_polys");
    return quotient_chunks_core(ctx, d_work, num_challenges, degree_bits, qbits, quotient_degree_factor, "quotient_polys", chunks_out);
}

extern "C" int p2hot_quotient_polys(p2hot_ctx *ctx, const p2hot_batch *wires, const p2hot_batch *constants_sigmas, size_t sigmas_first_col,
                                    const p2hot_batch *zs_partial_products, const uint64_t *k_is, unsigned num_routed,
                                    unsigned quotient_degree_factor, const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas,
                                    unsigned num_challenges, const uint64_t *const *gate_sums, uint64_t *values_out, p2hot_cols **chunks_out) {
    return quotient_polys_core(ctx, wires, constants_sigmas, sigmas_first_col, zs_partial_products, k_is, num_routed, quotient_degree_factor, betas,
                               gammas, alphas, num_challenges, gate_sums, values_out, chunks_out, nullptr);
}

// compute_quotient_polys (plonk/prover.rs:609-815) for a circuit with lookup tables: p2hot_quotient_polys plus
// check_lookup_constraints_batch's terms (plonk/vanishing_poly.rs:515-664) in their place of the term list (:317-322)
extern "C" int p2hot_quotient_polys_lookup(p2hot_ctx *ctx, const p2hot_batch *wires, const p2hot_batch *constants_sigmas, size_t sigmas_first_col,
                                           const p2hot_batch *zs_partial_products_lookups, const uint64_t *k_is, unsigned num_routed,
                                           unsigned quotient_degree_factor, const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas,
                                           unsigned num_challenges, const uint64_t *const *gate_sums, unsigned num_lu_slots, unsigned num_lut_slots,
                                           unsigned num_luts, size_t lookup_selectors_first_col, const uint64_t *deltas,
                                           const uint64_t *lut_re_poly_evals, uint64_t *values_out, p2hot_cols **chunks_out) {
    const LookupQuot lk{num_lu_slots, num_lut_slots, num_luts, lookup_selectors_first_col, deltas, lut_re_poly_evals};
    return quotient_polys_core(ctx, wires, constants_sigmas, sigmas_first_col, zs_partial_products_lookups, k_is, num_routed, quotient_degree_factor,
                               betas, gammas, alphas, num_challenges, gate_sums, values_out, chunks_out, &lk);
}

// p2hot_quotient_polys / p2hot_quotient_polys_lookup with evaluate_gate_constraints_base_batch (plonk/vanishing_poly.rs:702-728) for
// the gates of the set on the device; the host gate_sums is the residual of every other gate
extern "C" int p2hot_quotient_polys_gates(p2hot_ctx *ctx, const p2hot_batch *wires, const p2hot_batch *constants_sigmas, size_t sigmas_first_col,
                                          const p2hot_batch *zs_partial_products, const uint64_t *k_is, unsigned num_routed,
                                          unsigned quotient_degree_factor, const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas,
                                          unsigned num_challenges, const uint64_t *const *gate_sums, const p2hot_gate_set *gates,
                                          uint64_t *values_out, p2hot_cols **chunks_out) {
    return quotient_polys_core(ctx, wires, constants_sigmas, sigmas_first_col, zs_partial_products, k_is, num_routed, quotient_degree_factor, betas,
                               gammas, alphas, num_challenges, gate_sums, values_out, chunks_out, nullptr, gates, true);
}

extern "C" int p2hot_quotient_polys_lookup_gates(p2hot_ctx *ctx, const p2hot_batch *wires, const p2hot_batch *constants_sigmas, size_t sigmas_first_col,
                                                 const p2hot_batch *zs_partial_products_lookups, const uint64_t *k_is, unsigned num_routed,
                                                 unsigned quotient_degree_factor, const uint64_t *betas, const uint64_t *gammas,
                                                 const uint64_t *alphas, unsigned num_challenges, const uint64_t *const *gate_sums,
                                                 unsigned num_lu_slots, unsigned num_lut_slots, unsigned num_luts, size_t lookup_selectors_first_col,
                                                 const uint64_t *deltas, const uint64_t *lut_re_poly_evals, const p2hot_gate_set *gates,
                                                 uint64_t *values_out, p2hot_cols **chunks_out) {
    const LookupQuot lk{num_lu_slots, num_lut_slots, num_luts, lookup_selectors_first_col, deltas, lut_re_poly_evals};
    return quotient_polys_core(ctx, wires, constants_sigmas, sigmas_first_col, zs_partial_products_lookups, k_is, num_routed, quotient_degree_factor,
                               betas, gammas, alphas, num_challenges, gate_sums, values_out, chunks_out, &lk, gates, true);
}

// the two entry points above with the constraints of user-defined gates as gate programs (gate_program.hpp) beside the set's gates
extern "C" int p2hot_quotient_polys_gate_programs(p2hot_ctx *ctx, const p2hot_batch *wires, const p2hot_batch *constants_sigmas,
                                                  size_t sigmas_first_col, const p2hot_batch *zs_partial_products, const uint64_t *k_is,
                                                  unsigned num_routed, unsigned quotient_degree_factor, const uint64_t *betas,
                                                  const uint64_t *gammas, const uint64_t *alphas, unsigned num_challenges,
                                                  const uint64_t *const *gate_sums, const p2hot_gate_set *gates, uint64_t *values_out,
                                                  p2hot_cols **chunks_out, const p2hot_gate_program *programs, unsigned num_programs) {
    return quotient_polys_core(ctx, wires, constants_sigmas, sigmas_first_col, zs_partial_products, k_is, num_routed, quotient_degree_factor, betas,
                               gammas, alphas, num_challenges, gate_sums, values_out, chunks_out, nullptr, gates, true, programs, num_programs);
}

extern "C" int p2hot_quotient_polys_lookup_gate_programs(p2hot_ctx *ctx, const p2hot_batch *wires, const p2hot_batch *constants_sigmas,
                                                         size_t sigmas_first_col, const p2hot_batch *zs_partial_products_lookups,
                                                         const uint64_t *k_is, unsigned num_routed, unsigned quotient_degree_factor,
                                                         const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas,
                                                         unsigned num_challenges, const uint64_t *const *gate_sums, unsigned num_lu_slots,
                                                         unsigned num_lut_slots, unsigned num_luts, size_t lookup_selectors_first_col,
                                                         const uint64_t *deltas, const uint64_t *lut_re_poly_evals, const p2hot_gate_set *gates,
                                                         uint64_t *values_out, p2hot_cols **chunks_out, const p2hot_gate_program *programs,
                                                         unsigned num_programs) {
    const LookupQuot lk{num_lu_slots, num_lut_slots, num_luts, lookup_selectors_first_col, deltas, lut_re_poly_evals};
    return quotient_polys_core(ctx, wires, constants_sigmas, sigmas_first_col, zs_partial_products_lookups, k_is, num_routed, quotient_degree_factor,
                               betas, gammas, alphas, num_challenges, gate_sums, values_out, chunks_out, &lk, gates, true, programs, num_programs);
}

// ------------------------------------------------------------------ lookup polynomials (plonk/prover.rs:451-605)
extern "C" int p2hot_lookup_polys(p2hot_ctx *ctx, const p2hot_cols *wires, size_t wires_first_col, unsigned num_lu_slots, unsigned num_lut_slots,
                                  unsigned lookup_degree, const uint64_t *lookup_rows, unsigned num_luts, const uint64_t *deltas,
                                  unsigned num_challenges, uint64_t *out_host, p2hot_cols **out_cols) {
    P2_ENTER(ctx);
    if (out_cols) *out_cols = nullptr;
    if (!wires || wires->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "lookup_polys: null or foreign column set");
    if (!deltas || (num_luts && !lookup_rows)) P2_FAIL(ctx, P2HOT_EINVAL, "lookup_polys: null argument");
    if (num_challenges == 0 || num_challenges > 4) P2_FAIL(ctx, P2HOT_EINVAL, "lookup_polys: %u challenges (1..4)", num_challenges);
    if (lookup_degree == 0) P2_FAIL(ctx, P2HOT_EINVAL, "lookup_polys: lookup_degree is 0");
    if (num_lu_slots == 0 || num_lut_slots == 0) P2_FAIL(ctx, P2HOT_EINVAL, "lookup_polys: no lookup slots");
    if (wires_first_col > wires->W || (size_t)2 * num_lu_slots > wires->W - wires_first_col || (size_t)3 * num_lut_slots > wires->W - wires_first_col)
        P2_FAIL(ctx, P2HOT_EINVAL, "lookup_polys: %u LookupGate / %u LookupTableGate slots do not fit the wires given", num_lu_slots, num_lut_slots);
    const unsigned log_n = wires->log_n;
    const size_t n = (size_t)1 << log_n;
    size_t max_len = 1;
    for (unsigned r = 0; r < num_luts; ++r) {
        const uint64_t last_lu = lookup_rows[3 * r], last_lut = lookup_rows[3 * r + 1], first_lut = lookup_rows[3 * r + 2];
        if (!(last_lu <= last_lut && last_lut <= first_lut)) P2_FAIL(ctx, P2HOT_EINVAL, "lookup_polys: LUT %u: rows not ordered last_lu <= last_lut <= first_lut", r);
        // prover.rs:517: values[row + 1] at row = first_lut_row
        if (first_lut >= n || first_lut + 1 >= n) P2_FAIL(ctx, P2HOT_EINVAL, "lookup_polys: LUT %u: first_lut_gate + 1 = %llu is not a row of the trace", r, (unsigned long long)first_lut + 1);
        max_len = std::max(max_len, (size_t)(first_lut - last_lu + 1));
    }
    const unsigned S = (num_lu_slots + lookup_degree - 1) / lookup_degree;
    const size_t rows = (size_t)num_challenges * (S + 1), max_chunks = (max_len + lookup::SCAN_CHUNK - 1) / lookup::SCAN_CHUNK;
    PoolBuf d_out(ctx), d_sc(ctx);
    P2_TRY(pool_alloc(ctx, rows * n * 8, &d_out.p));
    P2_TRY(pool_alloc(ctx, 5 * (size_t)num_challenges * max_chunks * 8 + 8, &d_sc.p));
    lookup::PolyArgs a{};
    a.wires = wires->d + wires_first_col * n, a.wires_stride = n, a.out = d_out.u(), a.out_stride = n;
    a.num_lu_slots = num_lu_slots, a.num_lut_slots = num_lut_slots, a.lu_degree = lookup_degree, a.S = S;
    a.lut_degree = (num_lut_slots + S - 1) / S;  // prover.rs:473
    for (unsigned c = 0; c < num_challenges; ++c) {
        for (unsigned k = 0; k < 4; ++k) a.deltas[c][k] = gl::canon(deltas[(size_t)c * 4 + k]);
        a.delta_pow[c] = gl::pow(a.deltas[c][3], num_lut_slots);
    }
    unsigned *flag = (unsigned *)(d_sc.u() + 5 * (size_t)num_challenges * max_chunks);
    a.zero_flag = flag;
    unsigned zero = 0;
    auto body = [&]() -> int {
        ProfScope prof(ctx, "lookup_polys");
        P2_HIP(ctx, hipMemsetAsync(d_out.p, 0, rows * n * 8, ctx->stream));
        P2_HIP(ctx, hipMemsetAsync(flag, 0, 8, ctx->stream));
        // the regions one after the other, in the caller's order: each reads what the earlier ones left at its first_lut + 1
        for (unsigned r = 0; r < num_luts; ++r) {
            a.last_lu = lookup_rows[3 * r], a.last_lut = lookup_rows[3 * r + 1], a.first_lut = lookup_rows[3 * r + 2];
            const size_t len = a.first_lut - a.last_lu + 1;
            a.n_chunks = (len + lookup::SCAN_CHUNK - 1) / lookup::SCAN_CHUNK;
            const size_t stride = (size_t)num_challenges * a.n_chunks;
            a.csum = d_sc.u(), a.cmul = a.csum + stride, a.cadd = a.cmul + stride, a.carry_s = a.cadd + stride, a.carry_re = a.carry_s + stride;
            P2HOT_LAUNCH(lookup::lookup_rows_kernel, dim3(cdiv(len, 256), num_challenges), dim3(256), 0, ctx->stream, a);
            P2_LAUNCH_CHECK(ctx);
            P2HOT_LAUNCH(lookup::lookup_chunk_totals_kernel, dim3(cdiv(a.n_chunks, 64), num_challenges), dim3(64), 0, ctx->stream, a);
            P2_LAUNCH_CHECK(ctx);
            P2HOT_LAUNCH(lookup::lookup_carries_kernel, dim3(num_challenges), dim3(1024), 0, ctx->stream, a, (a.n_chunks + 1023) / 1024);
            P2_LAUNCH_CHECK(ctx);
            P2HOT_LAUNCH(lookup::lookup_emit_kernel, dim3(cdiv(a.n_chunks, 64), num_challenges), dim3(64), 0, ctx->stream, a);
            P2_LAUNCH_CHECK(ctx);
        }
        P2_HIP(ctx, hipMemcpyAsync(&zero, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
        if (out_host) P2_HIP(ctx, hipMemcpyAsync(out_host, d_out.p, rows * n * 8, hipMemcpyDeviceToHost, ctx->stream));
        return P2HOT_OK;
    };
    int rc = sync_checked(ctx, body(), "lookup_polys");
    if (rc != P2HOT_OK) return rc;
    if (zero) P2_FAIL(ctx, P2HOT_EINVAL, "lookup_polys: Tried to invert zero (alpha equals a looked or looking combination; the reference panics in batch_multiplicative_inverse)");
    if (out_cols) {
        *out_cols = new p2hot_cols{ctx, d_out.u(), rows, log_n, true};
        d_out.p = nullptr;
    }
    return rc;
}

// a's columns then b's as one new set (prover.rs:237-241: Zs / partial products ++ lookup polys go into ONE commitment); the
// inputs are left as they are
extern "C" int p2hot_cols_concat(p2hot_ctx *ctx, const p2hot_cols *a, const p2hot_cols *b, p2hot_cols **out) {
    P2_ENTER(ctx);
    if (!out) P2_FAIL(ctx, P2HOT_EINVAL, "cols_concat: null output");
    *out = nullptr;
    if (!a || !b || a->ctx != ctx || b->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "cols_concat: null or foreign column set");
    if (a->log_n != b->log_n) P2_FAIL(ctx, P2HOT_EINVAL, "cols_concat: the sets differ in degree (2^%u and 2^%u rows)", a->log_n, b->log_n);
    const size_t n = (size_t)1 << a->log_n;
    PoolBuf d(ctx);
    P2_TRY(pool_alloc(ctx, (a->W + b->W) * n * 8, &d.p));
    auto body = [&]() -> int {
        if (a->W) P2_HIP(ctx, hipMemcpyAsync(d.u(), a->d, a->W * n * 8, hipMemcpyDeviceToDevice, ctx->stream));
        if (b->W) P2_HIP(ctx, hipMemcpyAsync(d.u() + a->W * n, b->d, b->W * n * 8, hipMemcpyDeviceToDevice, ctx->stream));
        return P2HOT_OK;
    };
    P2_TRY(sync_checked(ctx, body(), "cols_concat"));
    *out = new p2hot_cols{ctx, d.u(), a->W + b->W, a->log_n, true};
    d.p = nullptr;
    return P2HOT_OK;
}

// ------------------------------------------------------------------ the middle of a proof for M witnesses of ONE circuit
// p2hot_commit_many and p2hot_prove_openings_many batch the two ends of M recursion-size proofs; these four batch what lies between:
// partial products and Zs, the commitment of an interleaved device column set, the quotient with its gate constraints, the
// OpeningSet.  Sigmas, constants, selectors, the gate set and k_is are shared; wires, challenges and the public-inputs hash are per
// proof and reach the kernels through a device table indexed by blockIdx.y (plonk::ManyProof, gates::ManyGate).  Every argument is
// checked before the first enqueue, a per-proof message names the proof, and each call synchronises once.

// where proof j's block lies from proof 0's, in words: the kernels add it to proof 0's pointer, which they have as an argument
static ptrdiff_t many_words_between(const u64 *p, const u64 *p0) { return (ptrdiff_t)(((intptr_t)p - (intptr_t)p0) / 8); }

// the per-proof checks the M-forms share: entry j of `tab` is a commitment of this context with `ref`'s degree and rate
static int many_check(p2hot_ctx *ctx, const char *what, const char *role, const p2hot_batch *const *tab, size_t M, const p2hot_batch *ref,
                      size_t min_width) {
    for (size_t j = 0; j < M; ++j) {
        const p2hot_batch *b = tab[j];
        if (!b) P2_FAIL(ctx, P2HOT_EINVAL, "%s: proof %zu: the %s commitment is null", what, j, role);
        if (b->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "%s: proof %zu: the %s commitment belongs to another context", what, j, role);
        if (!ref) ref = tab[0];
        if (b->log_n != ref->log_n || b->rate_bits != ref->rate_bits)
            P2_FAIL(ctx, P2HOT_EINVAL, "%s: proof %zu: the %s commitment differs in degree or rate (2^%u rows, rate 2^%u; expected 2^%u, 2^%u)", what, j,
                    role, b->log_n, b->rate_bits, ref->log_n, ref->rate_bits);
        if (b->W < min_width) P2_FAIL(ctx, P2HOT_EINVAL, "%s: proof %zu: the %s commitment has %zu polynomials, %zu are needed", what, j, role, b->W, min_width);
    }
    return P2HOT_OK;
}

extern "C" int p2hot_partial_products_many(p2hot_ctx *ctx, size_t M, const p2hot_batch *const *wires, size_t wires_first_col,
                                           const p2hot_cols *sigmas, size_t sigmas_first_col, const uint64_t *k_is, unsigned num_routed,
                                           unsigned degree, const uint64_t *betas, const uint64_t *gammas, unsigned num_challenges,
                                           uint64_t *out_host, p2hot_cols **out_cols) {
    P2_ENTER(ctx);
    const char *what = "partial_products_many";
    if (out_cols) *out_cols = nullptr;
    if (M == 0) return P2HOT_OK;
    if (!wires || !sigmas || !k_is || !betas || !gammas) P2_FAIL(ctx, P2HOT_EINVAL, "%s: null argument", what);
    if (sigmas->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "%s: the sigmas belong to another context", what);
    if (num_challenges == 0 || num_challenges > 4) P2_FAIL(ctx, P2HOT_EINVAL, "%s: %u challenges (1..4)", what, num_challenges);
    if (degree < 2 || !(degree < num_routed)) P2_FAIL(ctx, P2HOT_EINVAL, "%s: need 2 <= degree < num_routed", what);
    P2_TRY(many_check(ctx, what, "wires", wires, M, nullptr, wires_first_col + num_routed));
    const unsigned log_n = wires[0]->log_n, nc = num_challenges;
    if (sigmas->log_n != log_n) P2_FAIL(ctx, P2HOT_EINVAL, "%s: wires and sigmas have different lengths", what);
    if (sigmas_first_col > sigmas->W || num_routed > sigmas->W - sigmas_first_col)
        P2_FAIL(ctx, P2HOT_EINVAL, "%s: %u routed columns do not fit the sigmas", what, num_routed);
    if (M > 65535 || M * num_routed > 65535) P2_FAIL(ctx, P2HOT_EINVAL, "%s: M * num_routed = %zu polynomials exceed one launch (65535)", what, M * num_routed);
    const size_t n = (size_t)1 << log_n;
    const unsigned num_chunks = (num_routed + degree - 1) / degree, num_prods = num_chunks - 1;
    const size_t rows = (size_t)nc * (num_prods + 1);
    const unsigned chunk_log = log_n < 6 ? log_n : 6;  // rows per scan chunk (p2hot_partial_products_dev's)
    const size_t n_chunks = n >> chunk_log, per = (n_chunks + 1023) / 1024;
    // scratch: 2 x (chunk denominators [M][num_chunks][n] | row totals [M][n]) | chunk products [M][n_chunks] | carries | flags [M];
    // small: k_is | the per-proof table
    const size_t set_words = M * ((size_t)num_chunks * n + n), tab_words = M * sizeof(plonk::ManyProof) / 8;
    PoolBuf d_out(ctx), d_vals(ctx), d_scr(ctx), d_small(ctx);
    P2_TRY(pool_alloc(ctx, rows * M * n * 8, &d_out.p));
    P2_TRY(pool_alloc(ctx, M * num_routed * n * 8, &d_vals.p));
    P2_TRY(pool_alloc(ctx, (2 * set_words + 2 * M * n_chunks + M) * 8, &d_scr.p));
    P2_TRY(pool_alloc(ctx, (num_routed + tab_words) * 8, &d_small.p));
    std::vector<u64> small(num_routed + tab_words);
    for (unsigned j = 0; j < num_routed; ++j) small[j] = gl::canon(k_is[j]);
    plonk::ManyProof *tab = reinterpret_cast<plonk::ManyProof *>(small.data() + num_routed);
    for (size_t j = 0; j < M; ++j) {
        plonk::ManyProof t{};
        t.coef_off = many_words_between(wires[j]->d_coef, wires[0]->d_coef), t.coef_stride = wires[j]->col_stride_coef();
        for (unsigned c = 0; c < nc; ++c) t.betas[c] = gl::canon(betas[j * nc + c]), t.gammas[c] = gl::canon(gammas[j * nc + c]);
        tab[j] = t;
    }
    u64 *d_k = d_small.u(), *sets = d_scr.u(), *prod = sets + 2 * set_words, *carry = prod + M * n_chunks;
    unsigned *flags = (unsigned *)(carry + M * n_chunks);
    const plonk::ManyProof *d_tab = reinterpret_cast<const plonk::ManyProof *>(d_small.u() + num_routed);
    std::vector<unsigned> zero(M, 0);
    auto body = [&]() -> int {
        P2_HIP(ctx, hipMemcpyAsync(d_small.p, small.data(), small.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        P2_HIP(ctx, hipMemsetAsync(flags, 0, M * 8, ctx->stream));
        // the routed wires' values on H: a forward NTT of a copy of every proof's coefficients (p2hot_batch_subgroup_values' route)
        P2HOT_LAUNCH(plonk::many_gather_coeffs_kernel, dim3(cdiv(n, 256), num_routed, (unsigned)M), dim3(256), 0, ctx->stream, (const u64 *)wires[0]->d_coef, d_tab,
                     wires_first_col, n, d_vals.u());
        P2_LAUNCH_CHECK(ctx);
        P2_TRY(p2hot_fft_dev(ctx, d_vals.u(), M * num_routed, n, log_n));
        P2HOT_LAUNCH(ntt::canon_kernel, dim3(cdiv(M * num_routed * n, 256)), dim3(256), 0, ctx->stream, d_vals.u(), M * num_routed * n);
        P2_LAUNCH_CHECK(ctx);
        ProfScope ps(ctx, "partial_products_many");
        std::vector<plonk::PPArgs> args(nc);
        for (unsigned ch = 0; ch < nc; ++ch) {  // proof 0's blocks; the kernels step to proof blockIdx.y
            plonk::PPArgs &a = args[ch];
            u64 *dchunk = sets + (size_t)(ch & 1) * set_words;
            a.wires = d_vals.u(), a.wires_stride = n;
            a.sigmas = sigmas->d + sigmas_first_col * n, a.sigmas_stride = n;
            a.k_is = d_k;
            a.num_routed = num_routed, a.degree = degree, a.num_chunks = num_chunks, a.log_n = log_n;
            a.beta = a.gamma = 0;
            a.roots = ctx->fwd;
            a.pp = d_out.u() + ((size_t)nc + (size_t)ch * num_prods) * M * n;  // interleaved: column e of proof m is column e * M + m
            a.pp_stride = M * n;
            a.dchunk = dchunk;
            a.total = dchunk + M * (size_t)num_chunks * n;
            a.zero_flag = flags;
        }
        const dim3 grid(cdiv(n, 256), (unsigned)M);
        for (unsigned ch = 0; ch < nc; ++ch) {
            const plonk::PPArgs &a = args[ch];
            u64 *z = d_out.u() + (size_t)ch * M * n;
            if (ctx->pp_streams && (ch & 1) == 0 && ch + 1 < nc) {  // a pair of challenges in one pass, as the single-proof call runs them
                plonk::PPArgs2 two{{args[ch], args[ch + 1]}};
                P2HOT_LAUNCH(plonk::pp_quotients2_many_kernel, grid, dim3(256), 0, ctx->stream, two, d_tab, ch, (size_t)num_routed * n);
            } else if (!(ctx->pp_streams && (ch & 1))) {
                P2HOT_LAUNCH(plonk::pp_quotients_many_kernel, grid, dim3(256), 0, ctx->stream, a, d_tab, ch, (size_t)num_routed * n);
            }
            // the proofs' rows lie back to back: chunk totals, the Z walk and the scaling run over M * n rows, the carries restart per proof
            P2HOT_LAUNCH(plonk::pp_chunk_totals_kernel, dim3(cdiv(M * n_chunks, 256)), dim3(256), 0, ctx->stream, (const u64 *)a.total, chunk_log,
                         M * n_chunks, prod);
            P2HOT_LAUNCH(plonk::pp_carries_many_kernel, dim3(1, (unsigned)M), dim3(1024), 0, ctx->stream, (const u64 *)prod, n_chunks, per, carry);
            P2HOT_LAUNCH(plonk::pp_emit_z_kernel, dim3(cdiv(M * n_chunks, 256)), dim3(256), 0, ctx->stream, (const u64 *)a.total, chunk_log,
                         M * n_chunks, (const u64 *)carry, z);
            if (num_prods)
                P2HOT_LAUNCH(plonk::pp_scale_kernel, dim3(cdiv(M * n, 256)), dim3(256), 0, ctx->stream, a.pp, M * n, num_prods, (const u64 *)z, M * n);
            P2_LAUNCH_CHECK(ctx);
        }
        if (out_host)  // [M][rows][n] <- [rows][M][n]: one strided copy per proof
            for (size_t j = 0; j < M; ++j) P2_TRY(d2h_2d(ctx, out_host + j * rows * n, n * 8, d_out.u() + j * n, M * n * 8, n * 8, rows));
        P2_TRY(d2h(ctx, zero.data(), flags, M * 4));
        return P2HOT_OK;
    };
    int rc = sync_checked(ctx, body(), what);
    if (rc != P2HOT_OK) return rc;
    for (size_t j = 0; j < M; ++j)
        if (zero[j]) P2_FAIL(ctx, P2HOT_EINVAL, "%s: proof %zu: tried to invert zero (a denominator wire + beta*sigma + gamma vanished)", what, j);
    if (out_cols) {
        *out_cols = new p2hot_cols{ctx, d_out.u(), rows * M, log_n, true};
        d_out.p = nullptr;
    }
    return P2HOT_OK;
}

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
    if (M & (M - 1)) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: the number of proofs (%zu) must be a power of two", M);
    if (cols->W == 0) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: no polynomials (the reference panics on polynomials[0], fri/oracle.rs:90)");
    if (cols->W % M) P2_FAIL(ctx, P2HOT_EINVAL, "commit_cols_many: a set of %zu columns is not an interleaved set of %zu proofs", cols->W, M);
    if (cols->W > 65535) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: W * M = %zu polynomials exceed one launch (65535)", cols->W);
    if (cap_height > log_N) P2_FAIL(ctx, P2HOT_EINVAL, "commit_many: cap_height %u > log2(N) %u (merkle_tree.rs:195-200)", cap_height, log_N);
    unsigned lm = 0;
    while (((size_t)1 << lm) < M) ++lm;
    P2_TRY(check_log(ctx, log_N + lm, "commit_cols_many"));
    const size_t W = cols->W / M, n = (size_t)1 << log_n, N = n << rate_bits;
    const size_t nd = p2hot_num_digests(log_N, cap_height), cap_words = (size_t)4 << cap_height;
    PoolBuf d_co(ctx);
    d_co.p = cols->d;
    delete cols;  // consumed from here on: the block is ours whatever happens below
    PoolBuf d_lde(ctx), d_dig(ctx), d_cap(ctx);
    P2_TRY(pool_alloc(ctx, W * M * N * 8, &d_lde.p));
    P2_TRY(pool_alloc(ctx, (nd ? nd : 1) * M * 32, &d_dig.p));
    P2_TRY(pool_alloc(ctx, cap_words * M * 8, &d_cap.p));
    auto body = [&]() -> int {
        P2_TRY(p2hot_commit_many_dev(ctx, d_co.u(), M, W, log_n, rate_bits, cap_height, is_values, d_lde.u(), d_dig.u(), d_cap.u()));
        if (caps_out) P2_TRY(d2h(ctx, caps_out, d_cap.p, cap_words * M * 8));
        return P2HOT_OK;
    };
    int rc = sync_checked(ctx, body(), "commit_cols_many");
    if (rc == P2HOT_OK && handles_out) {  // p2hot_commit_many's handles: shares of the blocks, freed with the last one
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
    }
    return rc;
}

extern "C" int p2hot_quotient_polys_gates_many(p2hot_ctx *ctx, size_t M, const p2hot_batch *const *wires, const p2hot_batch *constants_sigmas,
                                               size_t sigmas_first_col, const p2hot_batch *const *zs_partial_products, const uint64_t *k_is,
                                               unsigned num_routed, unsigned quotient_degree_factor, const uint64_t *betas, const uint64_t *gammas,
                                               const uint64_t *alphas, unsigned num_challenges, const p2hot_gate_set *gs,
                                               const uint64_t *public_inputs_hashes, uint64_t *values_out, p2hot_cols **chunks_out) {
    P2_ENTER(ctx);
    const char *what = "quotient_polys_gates_many";
    if (chunks_out) *chunks_out = nullptr;
    if (M == 0) return P2HOT_OK;
    if (!wires || !constants_sigmas || !zs_partial_products || !k_is || !betas || !gammas || !alphas) P2_FAIL(ctx, P2HOT_EINVAL, "%s: null argument", what);
    if (!chunks_out && !values_out) P2_FAIL(ctx, P2HOT_EINVAL, "%s: nothing asked for", what);
    if (constants_sigmas->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "%s: the constants_sigmas commitment belongs to another context", what);
    const unsigned nc = num_challenges;
    if (nc == 0 || nc > 4) P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "%s: %u challenges (1..4 supported; plonky2's configs use 2)", what, nc);
    if (quotient_degree_factor < 2 || num_routed == 0) P2_FAIL(ctx, P2HOT_EINVAL, "%s: bad quotient degree factor or no routed wires", what);
    unsigned qbits = 0;
    while ((1u << qbits) < quotient_degree_factor) ++qbits;
    const unsigned num_chunks = (num_routed + quotient_degree_factor - 1) / quotient_degree_factor, num_prods = num_chunks - 1;
    P2_TRY(many_check(ctx, what, "wires", wires, M, constants_sigmas, num_routed));
    P2_TRY(many_check(ctx, what, "zs_partial_products", zs_partial_products, M, constants_sigmas, (size_t)nc * (1 + num_prods)));
    for (size_t j = 0; j < M; ++j)
        if (gs && wires[j]->col_stride_lde() >> 32)
            P2_FAIL(ctx, P2HOT_EINVAL, "%s: proof %zu: a wires column stride of %zu words (the gate kernels' M-form takes less than 2^32)", what, j,
                    wires[j]->col_stride_lde());
    for (size_t j = 1; j < M; ++j)
        if (wires[j]->W != wires[0]->W) P2_FAIL(ctx, P2HOT_EINVAL, "%s: proof %zu: %zu wires, proof 0 has %zu (one circuit)", what, j, wires[j]->W, wires[0]->W);
    if (qbits > constants_sigmas->rate_bits)
        P2_FAIL(ctx, P2HOT_EINVAL, "%s: quotient degree 2^%u above the rate 2^%u (prover.rs:632-636)", what, qbits, constants_sigmas->rate_bits);
    if (constants_sigmas->W < sigmas_first_col + num_routed) P2_FAIL(ctx, P2HOT_EINVAL, "%s: the constants_sigmas commitment is narrower than the permutation argument needs", what);
    if (M > 65535 || M * nc * quotient_degree_factor > 65535)
        P2_FAIL(ctx, P2HOT_EINVAL, "%s: W * M = %zu polynomials exceed one launch (65535)", what, M * nc * quotient_degree_factor);
    unsigned gs_stride = 0;
    if (gs) P2_TRY(gates_validate(ctx, gs, wires[0], constants_sigmas, sigmas_first_col, quotient_degree_factor, what, &gs_stride));
    const unsigned degree_bits = constants_sigmas->log_n, log_nq = degree_bits + qbits;
    P2_TRY(check_log(ctx, log_nq, what));
    const size_t n = (size_t)1 << degree_bits, m = n << qbits, rate = (size_t)1 << qbits, keep = n * quotient_degree_factor;
    // small: beta_c k_j [M][nc][num_routed] | Z_H and inverses [2 rate] | gate alpha powers [M][nc][gs_stride] | ManyProof [M] | ManyGate [M]
    const size_t nbk = M * nc * num_routed, n_gpow = M * nc * gs_stride, w_tab = M * sizeof(plonk::ManyProof) / 8, w_gtab = M * sizeof(gates::ManyGate) / 8;
    const size_t o_zh = nbk, o_gpow = o_zh + 2 * rate, o_tab = o_gpow + n_gpow, o_gtab = o_tab + w_tab;
    std::vector<u64> small(o_gtab + w_gtab);
    const u64 g_pow_n = gl::pow(gl::COSET_SHIFT, n), v = gl::root_of_unity(qbits);
    for (size_t j = 0; j < rate; ++j) {
        const u64 e = gl::canon(gl::sub(gl::mul(g_pow_n, gl::pow(v, j)), 1));
        if (e == 0) P2_FAIL(ctx, P2HOT_EINVAL, "%s: Z_H vanishes on the coset", what);
        small[o_zh + j] = e;
        small[o_zh + rate + j] = gl::inv(e);
    }
    const u64 K = (u64)nc + (u64)nc * num_chunks;
    plonk::ManyProof *tab = reinterpret_cast<plonk::ManyProof *>(small.data() + o_tab);
    gates::ManyGate *gtab = reinterpret_cast<gates::ManyGate *>(small.data() + o_gtab);
    for (size_t j = 0; j < M; ++j) {
        const uint64_t *be = betas + j * nc, *ga = gammas + j * nc, *al = alphas + j * nc;
        for (unsigned c = 0; c < nc; ++c)
            for (unsigned r = 0; r < num_routed; ++r) small[(j * nc + c) * num_routed + r] = gl::canon(gl::mul(be[c], k_is[r]));
        if (gs) gates_alpha_powers(small.data() + o_gpow + j * nc * gs_stride, al, nc, gs_stride);
        plonk::ManyProof t{};
        t.wires_off = many_words_between(wires[j]->d_lde, wires[0]->d_lde), t.wires_stride = wires[j]->col_stride_lde();
        t.zs_off = many_words_between(zs_partial_products[j]->d_lde, zs_partial_products[0]->d_lde), t.zs_stride = zs_partial_products[j]->col_stride_lde();
        for (unsigned a = 0; a < nc; ++a) {  // QuotArgs' per-challenge values, as quotient_polys_core fills them
            t.betas[a] = be[a], t.gammas[a] = gl::canon(ga[a]), t.alphas[a] = al[a];
            t.alpha_k[a] = gl::pow(al[a], K);
            for (unsigned c = 0; c < nc; ++c) t.base[a][c] = gl::pow(al[a], (u64)nc + (u64)c * num_chunks);
        }
        gates::ManyGate g{};
        g.wires_off = t.wires_off, g.wires_stride = (unsigned)t.wires_stride;
        g.wires = wires[j]->d_lde, g.wires_stride64 = t.wires_stride;
        for (unsigned k = 0; k < 4; ++k) {
            const u64 h = public_inputs_hashes ? public_inputs_hashes[j * 4 + k] : gs ? gs->public_inputs_hash[k] : 0;
            g.pih[k] = gl::canon(h);
        }
        tab[j] = t;
        gtab[j] = g;
    }
    PoolBuf d_work(ctx), d_small(ctx), d_gate(ctx), d_chunks(ctx);
    P2_TRY(pool_alloc(ctx, (M * nc * m + M) * 8, &d_work.p));  // the quotient values [M][nc][m], one flag word per proof behind them
    P2_TRY(pool_alloc(ctx, small.size() * 8, &d_small.p));
    if (gs) P2_TRY(pool_alloc(ctx, M * nc * m * 8, &d_gate.p));
    if (chunks_out) P2_TRY(pool_alloc(ctx, M * nc * quotient_degree_factor * n * 8, &d_chunks.p));
    // 1 / (n (x - 1)) for every point of the quotient coset: sizes only, kept by the context (quotient_polys_core's table)
    const auto inv_key = std::make_tuple(100, log_nq, qbits);
    auto inv_it = ctx->twid_cache.find(inv_key);
    if (inv_it == ctx->twid_cache.end()) {
        u64 *t = nullptr;
        P2_HIP(ctx, hipMalloc((void **)&t, m * 8));
        P2HOT_LAUNCH(plonk::quot_inv_kernel, dim3(cdiv(m, 256)), dim3(256), 0, ctx->stream, t, log_nq, (u64)n % gl::P, ctx->fwd);
        if (hipGetLastError() != hipSuccess) {
            (void)hipFree(t);
            P2_FAIL(ctx, P2HOT_EHIP, "%s: the L_0 denominator table could not be launched", what);
        }
        inv_it = ctx->twid_cache.emplace(inv_key, t).first;
    }
    plonk::QuotArgs q{};  // the shared fields and proof 0's matrices; the kernel takes the rest from the table
    q.wires = wires[0]->d_lde, q.zs = zs_partial_products[0]->d_lde;
    q.sigmas = constants_sigmas->d_lde + sigmas_first_col * constants_sigmas->col_stride_lde(), q.sigmas_stride = constants_sigmas->col_stride_lde();
    q.bk = d_small.u(), q.zh = d_small.u() + o_zh, q.inv_nx1 = inv_it->second;
    q.gate_sums = gs ? d_gate.u() : nullptr;
    q.out = d_work.u();
    q.num_routed = num_routed, q.degree = quotient_degree_factor, q.num_chunks = num_chunks, q.log_nq = log_nq, q.qbits = qbits;
    q.roots = ctx->fwd;
    const plonk::ManyProof *d_tab = reinterpret_cast<const plonk::ManyProof *>(d_small.u() + o_tab);
    const gates::ManyGate *d_gtab = reinterpret_cast<const gates::ManyGate *>(d_small.u() + o_gtab);
    unsigned *flags = (unsigned *)(d_work.u() + M * nc * m);
    std::vector<unsigned> nonzero(M, 0);
    auto body = [&]() -> int {
        P2_HIP(ctx, hipMemcpyAsync(d_small.p, small.data(), small.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        if (gs) {
            P2_HIP(ctx, hipMemsetAsync(d_gate.p, 0, M * nc * m * 8, ctx->stream));
            P2_TRY(gates_launch(ctx, gs, wires[0], constants_sigmas, d_small.u() + o_gpow, gs_stride, d_gate.u(), log_nq, nc, d_gtab, M));
        }
        {
            ProfScope prof(ctx, "quotient_perm_many");
            const dim3 grid(cdiv(m, 256), (unsigned)M), block(256);
            if (nc == 2 && quotient_degree_factor == 8) {  // the pipelined instantiation, as the single-proof call chooses it
                P2HOT_LAUNCH((plonk::quotient_perm_many_kernel<2, 8>), grid, block, 0, ctx->stream, q, d_tab);
            } else {
                switch (nc) {
                    case 1: P2HOT_LAUNCH((plonk::quotient_perm_many_kernel<1, 0>), grid, block, 0, ctx->stream, q, d_tab); break;
                    case 2: P2HOT_LAUNCH((plonk::quotient_perm_many_kernel<2, 0>), grid, block, 0, ctx->stream, q, d_tab); break;
                    case 3: P2HOT_LAUNCH((plonk::quotient_perm_many_kernel<3, 0>), grid, block, 0, ctx->stream, q, d_tab); break;
                    default: P2HOT_LAUNCH((plonk::quotient_perm_many_kernel<4, 0>), grid, block, 0, ctx->stream, q, d_tab); break;
                }
            }
            P2_LAUNCH_CHECK(ctx);
        }
        if (values_out) P2_HIP(ctx, hipMemcpyAsync(values_out, d_work.p, M * nc * m * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (!chunks_out) return P2HOT_OK;
        // values.coset_ifft(F::coset_shift()) on all M * nc polynomials, trim_to_len with one divisibility flag per proof, and the
        // chunks straight into the interleaved layout (quotient_chunks_core's steps)
        P2_TRY(p2hot_coset_ifft_dev(ctx, d_work.u(), M * nc, m, log_nq, gl::COSET_SHIFT));
        P2_HIP(ctx, hipMemsetAsync(flags, 0, M * 8, ctx->stream));
        if (keep < m) {
            P2HOT_LAUNCH(plonk::any_nonzero_many_kernel, dim3(cdiv(m - keep, 256), nc, (unsigned)M), dim3(256), 0, ctx->stream, (const u64 *)d_work.u(), m,
                         keep, flags);
            P2_LAUNCH_CHECK(ctx);
        }
        P2HOT_LAUNCH(plonk::chunks_interleave_kernel, dim3(cdiv(n, 256), nc * quotient_degree_factor, (unsigned)M), dim3(256), 0, ctx->stream,
                     (const u64 *)d_work.u(), m, n, quotient_degree_factor, nc, d_chunks.u());
        P2_LAUNCH_CHECK(ctx);
        P2_TRY(d2h(ctx, nonzero.data(), flags, M * 4));
        return P2HOT_OK;
    };
    int rc = sync_checked(ctx, body(), what);
    if (rc != P2HOT_OK) return rc;
    for (size_t j = 0; j < M; ++j)
        if (nonzero[j]) P2_FAIL(ctx, P2HOT_EINVAL, "Quotient has failed, the vanishing polynomial is not divisible by Z_H (proof %zu)", j);
    if (chunks_out) {
        *chunks_out = new p2hot_cols{ctx, d_chunks.u(), (size_t)nc * quotient_degree_factor * M, degree_bits, true};
        d_chunks.p = nullptr;
    }
    return P2HOT_OK;
}

extern "C" int p2hot_eval_openings_many(p2hot_ctx *ctx, size_t M, const p2hot_batch *const *batches, size_t n_batches, const uint64_t *points,
                                        size_t n_points, uint64_t *out) {
    P2_ENTER(ctx);
    const char *what = "eval_openings_many";
    if (M == 0 || n_batches == 0 || n_points == 0) return P2HOT_OK;
    if (!batches || !points || !out) P2_FAIL(ctx, P2HOT_EINVAL, "%s: null argument", what);
    if (M > 0x7FFFFFFFull / n_batches) P2_FAIL(ctx, P2HOT_EINVAL, "%s: too many oracles", what);
    for (size_t j = 0; j < M; ++j)
        for (size_t b = 0; b < n_batches; ++b) {
            const p2hot_batch *B = batches[j * n_batches + b];
            if (!B || B->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "%s: proof %zu: oracle %zu is null or belongs to another context", what, j, b);
            if (B->log_n != batches[0]->log_n)
                P2_FAIL(ctx, P2HOT_EINVAL, "%s: proof %zu: all oracles must have the same degree (oracle %zu: 2^%u vs 2^%u)", what, j, b, B->log_n,
                        batches[0]->log_n);
        }
    const unsigned log_n = batches[0]->log_n;
    P2_TRY(check_log(ctx, log_n, what));
    // every polynomial of every proof in order, with the proof it belongs to: one launch per stage for all proofs and points
    std::vector<const u64 *> ptrs;
    std::vector<unsigned> grp;
    for (size_t j = 0; j < M; ++j)
        for (size_t b = 0; b < n_batches; ++b) {
            const p2hot_batch *B = batches[j * n_batches + b];
            for (size_t c = 0; c < B->W; ++c) ptrs.push_back(B->d_coef + c * B->col_stride_coef()), grp.push_back((unsigned)j);
        }
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
    // the caller's layout: per proof, per oracle [n_points][W_o][2] (p2hot_eval_openings'), the proofs back to back
    size_t off = 0, out_off = 0;
    for (size_t j = 0; j < M; ++j)
        for (size_t b = 0; b < n_batches; ++b) {
            const size_t W = batches[j * n_batches + b]->W;
            for (size_t p = 0; p < n_points; ++p) std::copy(res.begin() + 2 * (p * total + off), res.begin() + 2 * (p * total + off + W), out + out_off + 2 * p * W);
            off += W;
            out_off += 2 * n_points * W;
        }
    return P2HOT_OK;
}
