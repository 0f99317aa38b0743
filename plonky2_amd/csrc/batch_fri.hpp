// batch_fri.hpp -- the mixed-degree batch FRI path of libp2hot (include/p2hot.h, "batch FRI" section).  Included at the end of
// p2hot.hip (one TU), after the plain FRI path whose building blocks it reuses.
//
// Reference call sites this layer stands behind:
//   BatchMerkleTree::new / open_batch / values       plonky2/src/hash/batch_merkle_tree.rs:35-130, :133-153, :155-164
//   BatchFriOracle::from_values / from_coeffs        batch_fri/oracle.rs:44-125        p2hot_batch_oracle_commit
//   batch_fri_committed_trees                        batch_fri/prover.rs:88-147        p2hot_batch_fri_commit_dev
//   BatchFriOracle::prove_openings + batch_fri_proof batch_fri/oracle.rs:128-192, batch_fri/prover.rs:25-86, :149-217
//                                                                                      p2hot_batch_prove_openings
#pragma once

#include <memory>

static const size_t kBatchMaxGroups = 8;  // fri::BatchTreeTable travels to the gather kernels by value

// heights strictly decreasing (batch_merkle_tree.rs:38-40), cap_height at most the last one (:42-48)
static int batch_tree_check(p2hot_ctx *ctx, const size_t *widths, const unsigned *log_heights, size_t n_groups, unsigned cap_height,
                            const char *what) {
    if (n_groups == 0) P2_FAIL(ctx, P2HOT_EINVAL, "%s: no groups (batch_merkle_tree.rs:36)", what);
    if (!widths || !log_heights) P2_FAIL(ctx, P2HOT_EINVAL, "%s: null widths / log_heights", what);
    if (n_groups > kBatchMaxGroups) P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "%s: %zu groups (at most %zu heights per tree)", what, n_groups, kBatchMaxGroups);
    P2_TRY(check_log(ctx, log_heights[0], what));
    for (size_t k = 0; k < n_groups; ++k) {
        if (k && log_heights[k] >= log_heights[k - 1])
            P2_FAIL(ctx, P2HOT_EINVAL, "%s: log_heights must decrease strictly (group %zu: %u after %u, batch_merkle_tree.rs:38-40)", what, k,
                    log_heights[k], log_heights[k - 1]);
        if (widths[k] > 0xFFFFFFF0ull) P2_FAIL(ctx, P2HOT_EINVAL, "%s: group %zu is too wide", what, k);
    }
    if (cap_height > log_heights[n_groups - 1])
        P2_FAIL(ctx, P2HOT_EINVAL, "%s: cap_height %u above the last group's height %u (batch_merkle_tree.rs:42-48)", what, cap_height,
                log_heights[n_groups - 1]);
    return P2HOT_OK;
}

// the tree as the gather kernels see it (d_groups / strides may be NULL for the paths kernel, which reads the digests only)
static fri::BatchTreeTable batch_tree_table(const uint64_t *const *d_groups, const size_t *strides, const size_t *widths,
                                            const unsigned *log_heights, size_t n_groups, unsigned cap_height) {
    fri::BatchTreeTable t{};
    t.n_groups = (unsigned)n_groups;
    size_t dig = 0;
    unsigned w = 0, layer = 0;
    for (size_t k = 0; k < n_groups; ++k) {
        const unsigned cap_k = k + 1 < n_groups ? log_heights[k + 1] : cap_height;
        t.lde[k] = d_groups ? d_groups[k] : nullptr;
        t.stride[k] = strides ? strides[k] : 0;
        t.dig_off[k] = dig;
        t.w_off[k] = w;
        t.shift[k] = log_heights[0] - log_heights[k];
        t.log_h[k] = log_heights[k];
        t.cap_h[k] = cap_k;
        t.layer_off[k] = layer;
        dig += 2 * (((size_t)1 << log_heights[k]) - ((size_t)1 << cap_k));
        w += widths ? (unsigned)widths[k] : 0;
        layer += log_heights[k] - cap_k;
    }
    t.total_w = w;
    t.layers = layer;
    return t;
}

// BatchMerkleTree::new: segment by segment through merkle_forest; the cap of segment k is the digest prefix of segment k + 1's leaves
static int batch_merkle_core(p2hot_ctx *ctx, const uint64_t *const *d_groups, const size_t *strides, const size_t *widths,
                             const unsigned *log_heights, size_t n_groups, unsigned cap_height, uint64_t *d_digests, uint64_t *d_cap) {
    P2_TRY(batch_tree_check(ctx, widths, log_heights, n_groups, cap_height, "batch_merkle"));
    if (!d_groups || !strides || !d_cap) P2_FAIL(ctx, P2HOT_EINVAL, "batch_merkle: null argument");
    if (p2hot_num_digests(log_heights[0], cap_height) && !d_digests) P2_FAIL(ctx, P2HOT_EINVAL, "batch_merkle: null digests");
    for (size_t k = 0; k < n_groups; ++k) {
        if (widths[k] && !d_groups[k]) P2_FAIL(ctx, P2HOT_EINVAL, "batch_merkle: group %zu is null", k);
        if (widths[k] && strides[k] < ((size_t)1 << log_heights[k])) P2_FAIL(ctx, P2HOT_EINVAL, "batch_merkle: group %zu: stride < rows", k);
    }
    const fri::BatchTreeTable t = batch_tree_table(d_groups, strides, widths, log_heights, n_groups, cap_height);
    // the caps between the segments: two buffers of 2^h_1 digests, used in turn
    u64 *mid[2] = {nullptr, nullptr};
    if (n_groups > 1) {
        const size_t words = (size_t)4 << log_heights[1];
        P2_TRY(scratch_get(ctx, 4, 2 * words * 8, (void **)&mid[0]));
        mid[1] = mid[0] + words;
    }
    for (size_t k = 0; k < n_groups; ++k) {
        u64 *cap_k = k + 1 < n_groups ? mid[k & 1] : d_cap;
        u64 *dig_k = d_digests ? d_digests + 4 * t.dig_off[k] : nullptr;
        const size_t rows = (size_t)1 << log_heights[k];
        if (k == 0)
            P2_TRY(merkle_forest(ctx, merkle::ColMajorReader{d_groups[0], strides[0]}, widths[0], log_heights[0], t.cap_h[0], 0, rows, dig_k,
                                 cap_k));
        else
            P2_TRY(merkle_forest(ctx, merkle::DigestPrefixedReader{mid[(k - 1) & 1], d_groups[k], strides[k]}, 4 + widths[k], log_heights[k],
                                 t.cap_h[k], 0, rows, dig_k, cap_k));
    }
    return P2HOT_OK;
}

extern "C" int p2hot_batch_merkle_dev(p2hot_ctx *ctx, const uint64_t *const *d_groups, const size_t *strides, const size_t *widths,
                                      const unsigned *log_heights, size_t n_groups, unsigned cap_height, uint64_t *d_digests,
                                      uint64_t *d_cap) {
    if (!ctx) return P2HOT_EINVAL;
    DeviceGuard dev_guard_(ctx);
    return batch_merkle_core(ctx, d_groups, strides, widths, log_heights, n_groups, cap_height, d_digests, d_cap);
}

static int batch_rows_launch(p2hot_ctx *ctx, const fri::BatchTreeTable &t, const u64 *d_idx, size_t m, u64 *d_out) {
    if (m == 0 || t.total_w == 0) return P2HOT_OK;
    P2HOT_LAUNCH(fri::batch_rows_kernel, dim3(cdiv(m * t.total_w, 256)), dim3(256), 0, ctx->stream, t, d_idx, m, d_out, ctx->d_oob);
    P2_LAUNCH_CHECK(ctx);
    return P2HOT_OK;
}

static int batch_paths_launch(p2hot_ctx *ctx, const u64 *d_digests, const fri::BatchTreeTable &t, const u64 *d_idx, size_t m, u64 *d_out) {
    if (m == 0 || t.layers == 0) return P2HOT_OK;
    P2HOT_LAUNCH(fri::batch_paths_kernel, dim3(cdiv(m * t.layers, 256)), dim3(256), 0, ctx->stream, d_digests, t, d_idx, m, d_out, ctx->d_oob);
    P2_LAUNCH_CHECK(ctx);
    return P2HOT_OK;
}

extern "C" int p2hot_batch_merkle_rows_dev(p2hot_ctx *ctx, const uint64_t *const *d_groups, const size_t *strides, const size_t *widths,
                                           const unsigned *log_heights, size_t n_groups, const uint64_t *d_idx, size_t m,
                                           uint64_t *d_out) {
    if (!ctx) return P2HOT_EINVAL;
    DeviceGuard dev_guard_(ctx);
    P2_TRY(batch_tree_check(ctx, widths, log_heights, n_groups, 0, "batch_merkle_rows"));
    if (!d_groups || !strides) P2_FAIL(ctx, P2HOT_EINVAL, "batch_merkle_rows: null argument");
    for (size_t k = 0; k < n_groups; ++k)
        if (widths[k] && (!d_groups[k] || strides[k] < ((size_t)1 << log_heights[k])))
            P2_FAIL(ctx, P2HOT_EINVAL, "batch_merkle_rows: group %zu is null or its stride < rows", k);
    const fri::BatchTreeTable t = batch_tree_table(d_groups, strides, widths, log_heights, n_groups, 0);
    if (m == 0 || t.total_w == 0) return P2HOT_OK;
    if (!d_idx || !d_out) P2_FAIL(ctx, P2HOT_EINVAL, "batch_merkle_rows: null pointer");
    return batch_rows_launch(ctx, t, d_idx, m, d_out);
}

extern "C" int p2hot_batch_merkle_paths_dev(p2hot_ctx *ctx, const uint64_t *d_digests, const unsigned *log_heights, size_t n_groups,
                                            unsigned cap_height, const uint64_t *d_idx, size_t m, uint64_t *d_out) {
    if (!ctx) return P2HOT_EINVAL;
    DeviceGuard dev_guard_(ctx);
    const size_t no_widths[kBatchMaxGroups] = {};
    P2_TRY(batch_tree_check(ctx, no_widths, log_heights, n_groups, cap_height, "batch_merkle_paths"));
    const fri::BatchTreeTable t = batch_tree_table(nullptr, nullptr, nullptr, log_heights, n_groups, cap_height);
    if (m == 0 || t.layers == 0) return P2HOT_OK;
    if (!d_digests || !d_idx || !d_out) P2_FAIL(ctx, P2HOT_EINVAL, "batch_merkle_paths: null pointer");
    return batch_paths_launch(ctx, d_digests, t, d_idx, m, d_out);
}

// ------------------------------------------------------------------ batch_fri_committed_trees
// the join schedule (batch_fri/prover.rs:39-50): after some round the folded degree bound must equal each later instance's
static int batch_join_check(p2hot_ctx *ctx, const unsigned *log_n, size_t n_instances, const unsigned *arity_bits, unsigned n_rounds,
                            const char *what) {
    if (n_instances == 0) P2_FAIL(ctx, P2HOT_EINVAL, "%s: n_instances = 0", what);
    if (!log_n || (n_rounds && !arity_bits)) P2_FAIL(ctx, P2HOT_EINVAL, "%s: null degree_bits / arity_bits", what);
    for (size_t j = 1; j < n_instances; ++j)
        if (log_n[j] >= log_n[j - 1])
            P2_FAIL(ctx, P2HOT_EINVAL, "%s: degree_bits must decrease strictly (instance %zu: %u after %u, batch_fri/prover.rs:36-38)", what, j,
                    log_n[j], log_n[j - 1]);
    unsigned cur = log_n[0];
    size_t next = 1;
    for (unsigned r = 0; r < n_rounds; ++r) {
        if (arity_bits[r] > cur) break;  // reported by the schedule check of the commit phase
        cur -= arity_bits[r];
        if (next < n_instances && cur == log_n[next]) ++next;
    }
    if (next != n_instances)
        P2_FAIL(ctx, P2HOT_EINVAL, "%s: instance %zu (degree 2^%u) is not reached exactly after a reduction round (batch_fri/prover.rs:50)", what,
                next, log_n[next]);
    return P2HOT_OK;
}

extern "C" int p2hot_batch_fri_commit_dev(p2hot_ctx *ctx, const uint64_t *const *d_coeffs_planar, const unsigned *log_n, size_t n_instances,
                                          unsigned rate_bits, unsigned cap_height, const unsigned *arity_bits, unsigned n_rounds,
                                          p2hot_challenger *challenger, uint64_t *d_leaves_out, uint64_t *digests_out,
                                          int digests_on_device, uint64_t *caps_out, uint64_t *betas_out, uint64_t *final_out) {
    if (!ctx || !challenger || challenger->ctx != ctx) return P2HOT_EINVAL;
    DeviceGuard dev_guard_(ctx);
    if (challenger->hash_n) P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "batch_fri_commit: batch FRI is Poseidon-only (the challenger is a KeccakHash<%u> one)", challenger->hash_n);
    P2_TRY(batch_join_check(ctx, log_n, n_instances, arity_bits, n_rounds, "batch_fri_commit"));
    if (!d_coeffs_planar) P2_FAIL(ctx, P2HOT_EINVAL, "batch_fri_commit: null coefficients");
    for (size_t j = 0; j < n_instances; ++j)
        if (!d_coeffs_planar[j]) P2_FAIL(ctx, P2HOT_EINVAL, "batch_fri_commit: the coefficients of instance %zu are null", j);
    const BatchJoin join{d_coeffs_planar + 1, log_n + 1, n_instances - 1};
    return fri_commit_core(ctx, nullptr, d_coeffs_planar[0], log_n[0], rate_bits, cap_height, arity_bits, n_rounds, 0, 0, challenger,
                           FriCommitOut{.leaves_out = d_leaves_out, .leaves_on_device = true, .digests_out = digests_out,
                                        .digests_on_device = digests_on_device != 0, .caps_out = caps_out, .betas_out = betas_out,
                                        .final_out = final_out},
                           &join);
}

// ------------------------------------------------------------------ BatchFriOracle, host pointers
struct p2hot_batch_oracle {
    p2hot_ctx *ctx;
    size_t W = 0;                  // polynomials
    std::vector<unsigned> log_n;   // per polynomial, non-increasing
    std::vector<size_t> coef_off;  // word offset of polynomial c in d_coef (W + 1 entries)
    unsigned rate_bits = 0, cap_height = 0;
    size_t n_groups = 0;
    size_t widths[kBatchMaxGroups] = {}, strides[kBatchMaxGroups] = {};  // polynomials of group k; rows of its LDE matrix
    unsigned log_heights[kBatchMaxGroups] = {};                          // degree log + rate_bits
    const uint64_t *d_groups[kBatchMaxGroups] = {};                      // group k's column-major LDE matrix inside d_lde
    u64 *d_coef = nullptr, *d_lde = nullptr, *d_dig = nullptr;
    fri::BatchTreeTable table() const { return batch_tree_table(d_groups, strides, widths, log_heights, n_groups, cap_height); }
};

extern "C" int p2hot_batch_oracle_commit(p2hot_ctx *ctx, const uint64_t *const *cols, const unsigned *log_n, size_t W, unsigned rate_bits,
                                         unsigned cap_height, int is_values, unsigned flags, uint64_t *coeffs_out, uint64_t *digests_out,
                                         uint64_t *cap_out, p2hot_batch_oracle **handle_out) {
    P2_ENTER(ctx);
    if (handle_out) *handle_out = nullptr;
    if (W == 0) P2_FAIL(ctx, P2HOT_EINVAL, "batch_oracle_commit: W = 0 (no polynomials)");
    if (!cols || !log_n) P2_FAIL(ctx, P2HOT_EINVAL, "batch_oracle_commit: null cols / log_n");
    if (flags & P2HOT_HASH_MASK) P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "batch_oracle_commit: batch FRI is Poseidon-only (flags %#x ask for a Keccak tree)", flags);
    if (flags) P2_FAIL(ctx, P2HOT_EINVAL, "batch_oracle_commit: unknown flags %#x", flags);
    std::unique_ptr<p2hot_batch_oracle> o(new p2hot_batch_oracle);
    o->ctx = ctx;
    o->W = W;
    o->rate_bits = rate_bits;
    o->cap_height = cap_height;
    size_t coef_words = 0, lde_words = 0;
    size_t lde_off[kBatchMaxGroups] = {}, first[kBatchMaxGroups] = {};
    for (size_t c = 0; c < W; ++c) {
        P2_TRY(check_log(ctx, log_n[c] + rate_bits, "batch_oracle_commit"));
        if (c && log_n[c] > log_n[c - 1])
            P2_FAIL(ctx, P2HOT_EINVAL, "batch_oracle_commit: log_n must not increase (polynomial %zu: %u after %u, batch_fri/oracle.rs:81)", c, log_n[c],
                    log_n[c - 1]);
        if (!cols[c]) P2_FAIL(ctx, P2HOT_EINVAL, "batch_oracle_commit: column %zu is null", c);
        if (c == 0 || log_n[c] != log_n[c - 1]) {
            if (o->n_groups == kBatchMaxGroups)
                P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "batch_oracle_commit: more than %zu different degrees", kBatchMaxGroups);
            first[o->n_groups] = c;
            o->log_heights[o->n_groups] = log_n[c] + rate_bits;
            o->strides[o->n_groups] = (size_t)1 << (log_n[c] + rate_bits);
            ++o->n_groups;
        }
        ++o->widths[o->n_groups - 1];
        o->log_n.push_back(log_n[c]);
        o->coef_off.push_back(coef_words);
        coef_words += (size_t)1 << log_n[c];
    }
    o->coef_off.push_back(coef_words);
    if (cap_height > log_n[W - 1] + rate_bits)
        P2_FAIL(ctx, P2HOT_EINVAL, "batch_oracle_commit: cap_height %u above the smallest LDE height %u (batch_merkle_tree.rs:42-48)", cap_height,
                log_n[W - 1] + rate_bits);
    uint64_t *const *coeffs_cols = reinterpret_cast<uint64_t *const *>(coeffs_out);
    if (coeffs_cols)
        for (size_t c = 0; c < W; ++c)
            if (!coeffs_cols[c]) P2_FAIL(ctx, P2HOT_EINVAL, "batch_oracle_commit: coefficient destination %zu is null", c);
    for (size_t k = 0; k < o->n_groups; ++k) {
        lde_off[k] = lde_words;
        lde_words += o->widths[k] * o->strides[k];
    }
    const size_t nd = p2hot_num_digests(o->log_heights[0], cap_height), cap_words = (size_t)4 << cap_height;
    PoolBuf d_coef(ctx), d_lde(ctx), d_dig(ctx), d_cap(ctx);
    P2_TRY(pool_alloc(ctx, coef_words * 8, &d_coef.p));
    P2_TRY(pool_alloc(ctx, lde_words * 8, &d_lde.p));
    P2_TRY(pool_alloc(ctx, (nd ? nd : 1) * 32, &d_dig.p));
    P2_TRY(pool_alloc(ctx, cap_words * 8, &d_cap.p));
    auto body = [&]() -> int {
        for (size_t k = 0; k < o->n_groups; ++k) {  // "IFFT" (oracle.rs:52-56) and "FFT + blinding", "transpose LDEs" (:89-101) per group
            const unsigned ln = o->log_n[first[k]];
            const size_t n = (size_t)1 << ln, Wk = o->widths[k];
            u64 *co = d_coef.u() + o->coef_off[first[k]];
            P2_TRY(h2d_columns(ctx, co, cols + first[k], Wk, n * 8, o->coef_off[first[k]] * 8, coef_words * 8, ctx->stream));
            if (is_values) P2_TRY(p2hot_ifft_dev(ctx, co, Wk, n, ln));
            P2HOT_LAUNCH(ntt::canon_kernel, dim3(cdiv(Wk * n, 256)), dim3(256), 0, ctx->stream, co, Wk * n);
            P2_LAUNCH_CHECK(ctx);
            o->d_groups[k] = d_lde.u() + lde_off[k];
            P2_TRY(p2hot_coset_lde_dev(ctx, co, Wk, n, ln, rate_bits, gl::COSET_SHIFT, 0, o->strides[k], d_lde.u() + lde_off[k], o->strides[k]));
        }
        if (coeffs_cols)
            for (size_t c = 0; c < W; ++c)
                P2_TRY(d2h(ctx, coeffs_cols[c], d_coef.u() + o->coef_off[c], ((size_t)8) << o->log_n[c]));
        // "build Field Merkle tree" (oracle.rs:108-112)
        P2_TRY(batch_merkle_core(ctx, o->d_groups, o->strides, o->widths, o->log_heights, o->n_groups, cap_height, d_dig.u(), d_cap.u()));
        if (digests_out && nd) P2_TRY(d2h(ctx, digests_out, d_dig.p, nd * 32));
        if (cap_out) P2_TRY(d2h(ctx, cap_out, d_cap.p, cap_words * 8));
        return P2HOT_OK;
    };
    P2_TRY(sync_checked(ctx, body(), "batch_oracle_commit"));
    if (handle_out) {
        o->d_coef = d_coef.u();
        o->d_lde = d_lde.u();
        o->d_dig = d_dig.u();
        d_coef.p = d_lde.p = d_dig.p = nullptr;  // ownership moves to the handle
        *handle_out = o.release();
    }
    return P2HOT_OK;
}

extern "C" size_t p2hot_batch_oracle_num_groups(const p2hot_batch_oracle *o) { return o ? o->n_groups : 0; }

extern "C" int p2hot_batch_oracle_group_info(const p2hot_batch_oracle *o, size_t group, size_t *width_out, unsigned *degree_log_out) {
    if (!o || group >= o->n_groups) return P2HOT_EINVAL;
    if (width_out) *width_out = o->widths[group];
    if (degree_log_out) *degree_log_out = o->log_heights[group] - o->rate_bits;
    return P2HOT_OK;
}

extern "C" int p2hot_batch_oracle_coeffs(p2hot_batch_oracle *o, size_t first, size_t count, uint64_t *out) {
    if (!o) return P2HOT_EINVAL;
    p2hot_ctx *ctx = o->ctx;
    P2_ENTER(ctx);
    if (first > o->W || count > o->W - first) P2_FAIL(ctx, P2HOT_EINVAL, "batch_oracle_coeffs: polynomials [%zu,+%zu) of %zu", first, count, o->W);
    if (count == 0) return P2HOT_OK;
    if (!out) P2_FAIL(ctx, P2HOT_EINVAL, "batch_oracle_coeffs: null output");
    // canonical since the commit (ntt::canon_kernel there)
    P2_HIP(ctx, hipMemcpyAsync(out, o->d_coef + o->coef_off[first], (o->coef_off[first + count] - o->coef_off[first]) * 8, hipMemcpyDeviceToHost,
                               ctx->stream));
    return sync_checked(ctx, P2HOT_OK, "batch_oracle_coeffs");
}

extern "C" int p2hot_batch_oracle_digests(p2hot_batch_oracle *o, uint64_t *out) {
    if (!o) return P2HOT_EINVAL;
    p2hot_ctx *ctx = o->ctx;
    P2_ENTER(ctx);
    const size_t nd = p2hot_num_digests(o->log_heights[0], o->cap_height);
    if (nd == 0) return P2HOT_OK;
    if (!out) P2_FAIL(ctx, P2HOT_EINVAL, "batch_oracle_digests: null output");
    P2_HIP(ctx, hipMemcpyAsync(out, o->d_dig, nd * 32, hipMemcpyDeviceToHost, ctx->stream));
    return sync_checked(ctx, P2HOT_OK, "batch_oracle_digests");
}

// rows (paths == false) or paths of m host-resident leaf indices
static int batch_oracle_open(p2hot_batch_oracle *o, const uint64_t *idx, size_t m, uint64_t *out, bool paths, const char *what) {
    p2hot_ctx *ctx = o->ctx;
    P2_ENTER(ctx);
    const fri::BatchTreeTable t = o->table();
    const size_t per = paths ? 4 * (size_t)t.layers : t.total_w;
    if (m == 0 || per == 0) return P2HOT_OK;
    if (!idx || !out) P2_FAIL(ctx, P2HOT_EINVAL, "%s: null buffer", what);
    for (size_t i = 0; i < m; ++i)
        if (idx[i] >> o->log_heights[0]) P2_FAIL(ctx, P2HOT_EINVAL, "%s: index %llu out of range", what, (unsigned long long)idx[i]);
    PoolBuf d_idx(ctx), d_out(ctx);
    P2_TRY(pool_alloc(ctx, m * 8, &d_idx.p));
    P2_TRY(pool_alloc(ctx, m * per * 8, &d_out.p));
    auto body = [&]() -> int {
        P2_HIP(ctx, hipMemcpyAsync(d_idx.p, idx, m * 8, hipMemcpyHostToDevice, ctx->stream));
        if (paths)
            P2_TRY(batch_paths_launch(ctx, o->d_dig, t, d_idx.u(), m, d_out.u()));
        else
            P2_TRY(batch_rows_launch(ctx, t, d_idx.u(), m, d_out.u()));
        return d2h(ctx, out, d_out.p, m * per * 8);
    };
    return sync_checked(ctx, body(), what);
}

extern "C" int p2hot_batch_oracle_rows(p2hot_batch_oracle *o, const uint64_t *row_idx, size_t m, uint64_t *out) {
    return o ? batch_oracle_open(o, row_idx, m, out, false, "batch_oracle_rows") : P2HOT_EINVAL;
}

extern "C" int p2hot_batch_oracle_paths(p2hot_batch_oracle *o, const uint64_t *leaf_idx, size_t m, uint64_t *out) {
    return o ? batch_oracle_open(o, leaf_idx, m, out, true, "batch_oracle_paths") : P2HOT_EINVAL;
}

extern "C" void p2hot_batch_oracle_free(p2hot_batch_oracle *o) {
    if (!o) return;
    (void)hipStreamSynchronize(o->ctx->stream);
    pool_release(o->ctx, o->d_lde);
    pool_release(o->ctx, o->d_dig);
    pool_release(o->ctx, o->d_coef);
    delete o;
}

// ------------------------------------------------------------------ BatchFriOracle::prove_openings + batch_fri_proof
extern "C" int p2hot_batch_fri_proof_sizes(const p2hot_batch_oracle *const *oracles, size_t n_oracles, const p2hot_fri_params *fp,
                                           p2hot_fri_proof_layout *out) {
    if (!oracles || n_oracles == 0 || !oracles[0]) return P2HOT_EINVAL;
    std::vector<size_t> widths;
    for (size_t o = 0; o < n_oracles; ++o) {
        if (!oracles[o]) return P2HOT_EINVAL;
        widths.push_back(oracles[o]->W);
    }
    return fri_proof_layout(widths.data(), n_oracles, oracles[0]->log_n[0], fp, out);
}

extern "C" int p2hot_batch_prove_openings(p2hot_ctx *ctx, const unsigned *degree_bits, const p2hot_fri_instance *instances, size_t n_instances,
                                          const p2hot_batch_oracle *const *oracles, size_t n_oracles, p2hot_challenger *challenger,
                                          const p2hot_fri_params *fp, p2hot_fri_proof *proof) {
    P2_ENTER(ctx);
    const char *const what = "batch_prove_openings";
    // --- validation: nothing is enqueued before all of it has passed
    if (!challenger || challenger->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "%s: the challenger is null or belongs to another context", what);
    if (challenger->hash_n)
        P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "%s: batch FRI is Poseidon-only (the challenger is a KeccakHash<%u> one)", what, challenger->hash_n);
    if (!fp) P2_FAIL(ctx, P2HOT_EINVAL, "%s: null fri params", what);
    if (!proof || !oracles || n_oracles == 0) P2_FAIL(ctx, P2HOT_EINVAL, "%s: null proof / oracles", what);
    if (n_instances == 0) P2_FAIL(ctx, P2HOT_EINVAL, "%s: n_instances = 0", what);
    if (!degree_bits || !instances) P2_FAIL(ctx, P2HOT_EINVAL, "%s: null degree_bits / instances", what);
    if (fp->max_num_query_steps || fp->final_poly_coeff_len)
        P2_FAIL(ctx, P2HOT_EINVAL, "%s: max_num_query_steps / final_poly_coeff_len do not exist on the batch path (batch_fri/prover.rs:88-97)", what);
    P2_TRY(batch_join_check(ctx, degree_bits, n_instances, fp->reduction_arity_bits, fp->n_reduction_rounds, what));
    const unsigned rate_bits = fp->rate_bits, cap_height = fp->cap_height, log_N = degree_bits[0] + rate_bits;
    std::vector<size_t> leaf_widths;
    for (size_t o = 0; o < n_oracles; ++o) {
        const p2hot_batch_oracle *B = oracles[o];
        if (!B || B->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "%s: oracle %zu is null or belongs to another context", what, o);
        if (B->rate_bits != rate_bits || B->cap_height != cap_height)
            P2_FAIL(ctx, P2HOT_EINVAL, "%s: oracle %zu was committed with another rate / cap height", what, o);
        if (B->log_heights[0] != log_N)
            P2_FAIL(ctx, P2HOT_EINVAL, "%s: the tallest group of oracle %zu has 2^%u rows, not 2^(degree_bits[0] + rate_bits) = 2^%u", what, o,
                    B->log_heights[0], log_N);
        leaf_widths.push_back(B->W);
    }
    // the polynomial table of every instance (FriInstanceInfo.batches): device pointers in batch order
    std::vector<OpeningInstance> tables(n_instances);
    for (size_t i = 0; i < n_instances; ++i) {
        OpeningInstance &in = tables[i];
        in.log_n = degree_bits[i];
        if (instances[i].n_batches && !instances[i].batches) P2_FAIL(ctx, P2HOT_EINVAL, "%s: instance %zu has null batches", what, i);
        for (size_t b = 0; b < instances[i].n_batches; ++b) {
            const p2hot_fri_batch_info &bi = instances[i].batches[b];
            if (bi.n_polys && (!bi.oracle_index || !bi.poly_index))
                P2_FAIL(ctx, P2HOT_EINVAL, "%s: instance %zu batch %zu has null index arrays", what, i, b);
            for (size_t j = 0; j < bi.n_polys; ++j) {
                const size_t oi = bi.oracle_index[j], pi = bi.poly_index[j];
                if (oi >= n_oracles || pi >= oracles[oi]->W)
                    P2_FAIL(ctx, P2HOT_EINVAL, "%s: instance %zu batch %zu opens polynomial (%zu, %zu) which does not exist", what, i, b, oi, pi);
                if (oracles[oi]->log_n[pi] != degree_bits[i])
                    P2_FAIL(ctx, P2HOT_EINVAL, "%s: instance %zu opens polynomial (%zu, %zu) of degree 2^%u, not 2^degree_bits[%zu] = 2^%u "
                            "(batch_fri/oracle.rs:170)", what, i, oi, pi, oracles[oi]->log_n[pi], i, degree_bits[i]);
                in.ptrs.push_back(oracles[oi]->d_coef + oracles[oi]->coef_off[pi]);
            }
            in.offsets.push_back(in.ptrs.size());
            in.points.push_back(bi.point[0]);
            in.points.push_back(bi.point[1]);
        }
    }
    // batch_fri/prover.rs:186-198: per oracle (values(x) flattened, open_batch(x)); the rest is the plain opening proof with the
    // later instances joining the commit phase (prove_openings_core)
    const DeviceOpener on_device = [&](size_t o, const u64 *d_idx, size_t Q, u64 *d_rows, u64 *d_paths) -> int {
        const fri::BatchTreeTable t = oracles[o]->table();
        P2_TRY(batch_rows_launch(ctx, t, d_idx, Q, d_rows));
        return batch_paths_launch(ctx, oracles[o]->d_dig, t, d_idx, Q, d_paths);
    };
    return prove_openings_core(ctx, what, tables, leaf_widths, &on_device, nullptr, challenger, fp, proof);
}
