// host_stark.hpp -- the host-pointer entry points of starky's lookup and cross-table-lookup stage (include/p2hot.h, "starky"
// section; kernels in stark.hpp).  Included at the end of p2hot.hip (one TU).
//
// Reference call sites this layer stands behind (starky/src):
//   lookup_helper_columns per lookup and challenge    prover.rs:177-195, lookup.rs:579-652              p2hot_stark_lookup_polys
//   cross_table_lookup_data / partial_sums            cross_table_lookup.rs:270-414                     p2hot_stark_ctl_polys
//   compute_quotient_polys, the arguments' terms      prover.rs:488-671, lookup.rs:804-863,
//                                                     cross_table_lookup.rs:558-629                     p2hot_stark_quotient_polys
//   ... with Stark::eval_packed_generic as a constraint program (host_air.hpp, air.hpp)                 p2hot_stark_quotient_polys_air
//   the program's consumer accumulators alone                                                           p2hot_stark_constraint_accs
#pragma once

namespace {
// the caller's descriptors, checked and canonical, and what the kernels need besides: every lookup under every challenge and
// every CTL Z as one stark::ZDesc (lookups first), the aux columns' layout, the map from helper columns to chunks
struct StarkPlan {
    std::vector<p2hot_stark_term> terms;
    std::vector<p2hot_stark_column> columns;
    std::vector<u32> products, constants;
    std::vector<p2hot_stark_filter> filters;
    std::vector<p2hot_stark_looking> entries;  // the caller's looking entries, then one per looking column of every lookup
    std::vector<stark::ZDesc> zs;
    std::vector<stark::HelperMap> hmap;
    unsigned chunk = 1;
    size_t num_lookup_cols = 0, num_ctl_helpers = 0, num_cols = 0;
    unsigned K = 0;  // the quotient's term count
    std::vector<u64> blob;  // host image of the device block (outlives the asynchronous copy)
};
}  // namespace

// every check of the descriptors, before anything is enqueued (include/p2hot.h lists them)
static int stark_plan(p2hot_ctx *ctx, const char *what, const p2hot_stark_tables *tb, size_t trace_width, const p2hot_stark_lookup *lookups,
                      unsigned num_lookups, const uint64_t *challenges, unsigned nc, const p2hot_stark_ctl_z *ctl_zs, unsigned num_zs,
                      const unsigned *ctl_num_helpers, unsigned constraint_degree, StarkPlan *pl) {
    if (nc == 0 || nc > 4) P2_FAIL(ctx, P2HOT_EINVAL, "%s: %u challenges (1..4)", what, nc);
    // constraint_degree.checked_sub(1).unwrap_or(1) (lookup.rs:439, :670, :755); 1 - 1 = 0 divides by zero there
    if (constraint_degree == 1) P2_FAIL(ctx, P2HOT_EINVAL, "%s: constraint_degree 1 (chunks of constraint_degree - 1 = 0 columns)", what);
    pl->chunk = constraint_degree ? constraint_degree - 1 : 1;
    if ((num_lookups && (!lookups || !challenges)) || (num_zs && !ctl_zs)) P2_FAIL(ctx, P2HOT_EINVAL, "%s: null argument", what);
    if (!tb) {
        if (num_lookups || num_zs) P2_FAIL(ctx, P2HOT_EINVAL, "%s: null descriptor tables", what);
        return P2HOT_OK;
    }
    if ((tb->num_terms && !tb->terms) || (tb->num_columns && !tb->columns) || (tb->num_products && !tb->products) ||
        (tb->num_constants && !tb->constants) || (tb->num_filters && !tb->filters) || (tb->num_looking && !tb->looking))
        P2_FAIL(ctx, P2HOT_EINVAL, "%s: a descriptor array is null but its count is not", what);
    auto fits = [](u32 first, u32 count, u32 size) { return first <= size && count <= size - first; };
    pl->terms.assign(tb->terms, tb->terms + tb->num_terms);
    for (u32 k = 0; k < tb->num_terms; ++k) {
        p2hot_stark_term &t = pl->terms[k];
        if (t.col >= trace_width) P2_FAIL(ctx, P2HOT_EINVAL, "%s: term %u reads column %u of a trace of %zu", what, k, t.col, trace_width);
        if (t.next > 1) P2_FAIL(ctx, P2HOT_EINVAL, "%s: term %u: next = %u (0 or 1)", what, k, t.next);
        t.coeff = gl::canon(t.coeff);
    }
    pl->columns.assign(tb->columns, tb->columns + tb->num_columns);
    for (u32 k = 0; k < tb->num_columns; ++k) {
        p2hot_stark_column &c = pl->columns[k];
        if (!fits(c.first_term, c.num_terms, tb->num_terms)) P2_FAIL(ctx, P2HOT_EINVAL, "%s: column %u: terms [%u, +%u) of %u", what, k, c.first_term, c.num_terms, tb->num_terms);
        c.constant = gl::canon(c.constant);
    }
    pl->products.assign(tb->products, tb->products + 2 * (size_t)tb->num_products);
    pl->constants.assign(tb->constants, tb->constants + tb->num_constants);
    for (u32 id : pl->products)
        if (id >= tb->num_columns) P2_FAIL(ctx, P2HOT_EINVAL, "%s: a filter product names column %u of %u", what, id, tb->num_columns);
    for (u32 id : pl->constants)
        if (id >= tb->num_columns) P2_FAIL(ctx, P2HOT_EINVAL, "%s: a filter constant names column %u of %u", what, id, tb->num_columns);
    pl->filters.assign(tb->filters, tb->filters + tb->num_filters);
    for (u32 k = 0; k < tb->num_filters; ++k) {
        const p2hot_stark_filter &f = pl->filters[k];
        if (!fits(f.first_product, f.num_products, tb->num_products) || !fits(f.first_constant, f.num_constants, tb->num_constants))
            P2_FAIL(ctx, P2HOT_EINVAL, "%s: filter %u: products [%u, +%u) of %u, constants [%u, +%u) of %u", what, k, f.first_product, f.num_products,
                    tb->num_products, f.first_constant, f.num_constants, tb->num_constants);
    }
    pl->entries.assign(tb->looking, tb->looking + tb->num_looking);
    for (u32 k = 0; k < tb->num_looking; ++k) {
        const p2hot_stark_looking &e = pl->entries[k];
        if (!fits(e.first_column, e.num_columns, tb->num_columns) || e.filter >= tb->num_filters)
            P2_FAIL(ctx, P2HOT_EINVAL, "%s: looking entry %u: columns [%u, +%u) of %u, filter %u of %u", what, k, e.first_column, e.num_columns,
                    tb->num_columns, e.filter, tb->num_filters);
    }
    const unsigned chunk = pl->chunk;
    // the lookups, each under every challenge (prover.rs:183-192): H helper columns, then Z
    size_t pos = 0;
    for (unsigned l = 0; l < num_lookups; ++l) {
        const p2hot_stark_lookup &lk = lookups[l];
        if (lk.num_columns == 0) P2_FAIL(ctx, P2HOT_EINVAL, "%s: lookup %u has no looking column", what, l);
        if (!fits(lk.first_column, lk.num_columns, tb->num_columns) || !fits(lk.first_filter, lk.num_columns, tb->num_filters) ||
            lk.table_column >= tb->num_columns || lk.frequencies_column >= tb->num_columns)
            P2_FAIL(ctx, P2HOT_EINVAL, "%s: lookup %u: columns [%u, +%u) of %u, filters from %u of %u, table %u, frequencies %u", what, l,
                    lk.first_column, lk.num_columns, tb->num_columns, lk.first_filter, tb->num_filters, lk.table_column, lk.frequencies_column);
        if (chunk >= 3 && lk.num_columns >= 3)
            P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "%s: lookup %u has a chunk of three or more columns (eval_helper_columns: todo!, lookup.rs:691)", what, l);
        const u32 first_entry = (u32)pl->entries.size(), H = (lk.num_columns + chunk - 1) / chunk;
        for (u32 j = 0; j < lk.num_columns; ++j) pl->entries.push_back(p2hot_stark_looking{lk.first_column + j, 1, lk.first_filter + j});
        for (unsigned c = 0; c < nc; ++c) {
            pl->zs.push_back(stark::ZDesc{first_entry, lk.num_columns, H, (u32)pos, (u32)(pos + H), 0, lk.table_column, lk.frequencies_column, 1,
                                          gl::canon(challenges[c])});
            pos += H + 1;
            pl->K += H + 2;
        }
    }
    pl->num_lookup_cols = pos;
    // the CTL Zs (cross_table_lookup.rs:253-261): the helper columns of all of them, then the Zs
    std::vector<u32> nh(num_zs);
    for (unsigned k = 0; k < num_zs; ++k) {
        const p2hot_stark_ctl_z &z = ctl_zs[k];
        if (z.num_looking == 0) P2_FAIL(ctx, P2HOT_EINVAL, "%s: CTL Z %u has no looking entry", what, k);
        if (!fits(z.first_looking, z.num_looking, tb->num_looking))
            P2_FAIL(ctx, P2HOT_EINVAL, "%s: CTL Z %u: looking entries [%u, +%u) of %u", what, k, z.first_looking, z.num_looking, tb->num_looking);
        if (chunk >= 3 && z.num_looking >= 3)
            P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "%s: CTL Z %u has a chunk of three or more entries (eval_helper_columns: todo!, lookup.rs:691)", what, k);
        const u32 full = (z.num_looking + chunk - 1) / chunk;
        nh[k] = ctl_num_helpers ? ctl_num_helpers[k] : (z.num_looking > 1 ? full : 0);  // cross_table_lookup.rs:407-411
        if (nh[k] != 0 && nh[k] != full) P2_FAIL(ctx, P2HOT_EINVAL, "%s: CTL Z %u: %u helper columns for %u entries in chunks of %u", what, k, nh[k], z.num_looking, chunk);
        if (nh[k] == 0 && z.num_looking > 2) P2_FAIL(ctx, P2HOT_EINVAL, "%s: CTL Z %u: %u entries need helper columns", what, k, z.num_looking);
        pl->num_ctl_helpers += nh[k];
    }
    size_t hpos = pl->num_lookup_cols;
    for (unsigned k = 0; k < num_zs; ++k) {
        const p2hot_stark_ctl_z &z = ctl_zs[k];
        pl->zs.push_back(stark::ZDesc{z.first_looking, z.num_looking, nh[k], (u32)hpos, (u32)(pl->num_lookup_cols + pl->num_ctl_helpers + k), 1, 0, 0,
                                      gl::canon(z.beta), gl::canon(z.gamma)});
        hpos += nh[k];
        pl->K += nh[k] + 2;
    }
    pl->num_cols = pl->num_lookup_cols + pl->num_ctl_helpers + num_zs;
    for (size_t zi = 0; zi < pl->zs.size(); ++zi) {
        const stark::ZDesc &z = pl->zs[zi];
        for (u32 k = 0; k < z.num_helpers; ++k)
            pl->hmap.push_back(stark::HelperMap{(u32)zi, z.first_entry + k * chunk, std::min(chunk, z.num_entries - k * chunk), z.helper_col + k});
        if (z.kind == 1 && z.num_helpers == 0) pl->hmap.push_back(stark::HelperMap{(u32)zi, z.first_entry, z.num_entries, z.z_col});
    }
    if (pl->hmap.size() > 65535 || pl->zs.size() > 65535) P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "%s: more than 65535 helper columns or Zs in one call", what);
    return P2HOT_OK;
}

// the plan's arrays as one device block (8-byte aligned pieces); *t points into it
static size_t stark_blob_layout(StarkPlan &pl, u64 *d_base, stark::Tables *t) {
    size_t words = 0;
    auto place = [&](const void *src, size_t bytes) -> const void * {
        const size_t at = words, w = (bytes + 7) / 8;
        words += w ? w : 1;
        if (d_base) {
            if (bytes) memcpy((unsigned char *)(pl.blob.data() + at), src, bytes);
            return d_base + at;
        }
        return nullptr;
    };
    t->terms = (const p2hot_stark_term *)place(pl.terms.data(), pl.terms.size() * sizeof(p2hot_stark_term));
    t->columns = (const p2hot_stark_column *)place(pl.columns.data(), pl.columns.size() * sizeof(p2hot_stark_column));
    t->products = (const u32 *)place(pl.products.data(), pl.products.size() * 4);
    t->constants = (const u32 *)place(pl.constants.data(), pl.constants.size() * 4);
    t->filters = (const p2hot_stark_filter *)place(pl.filters.data(), pl.filters.size() * sizeof(p2hot_stark_filter));
    t->entries = (const p2hot_stark_looking *)place(pl.entries.data(), pl.entries.size() * sizeof(p2hot_stark_looking));
    t->zs = (const stark::ZDesc *)place(pl.zs.data(), pl.zs.size() * sizeof(stark::ZDesc));
    t->hmap = (const stark::HelperMap *)place(pl.hmap.data(), pl.hmap.size() * sizeof(stark::HelperMap));
    return words;
}

static int stark_blob_alloc(p2hot_ctx *ctx, StarkPlan &pl, PoolBuf &d, stark::Tables *t) {
    const size_t words = stark_blob_layout(pl, nullptr, t);
    pl.blob.assign(words, 0);
    P2_TRY(pool_alloc(ctx, words * 8, &d.p));
    stark_blob_layout(pl, d.u(), t);
    return P2HOT_OK;
}

// get_helper_cols + the running sums for every ZDesc of the plan into a new column set of plan.num_cols columns
static int stark_aux_polys(p2hot_ctx *ctx, const char *what, const p2hot_cols *trace, StarkPlan &pl, uint64_t *out_host, p2hot_cols **out_cols,
                           uint64_t *zs_first, size_t first_z_col, unsigned num_zs_first) {
    const unsigned log_n = trace->log_n;
    const size_t n = (size_t)1 << log_n, n_chunks = (n + stark::SCAN_CHUNK - 1) / stark::SCAN_CHUNK, num_z = pl.zs.size();
    PoolBuf d_out(ctx), d_desc(ctx), d_sc(ctx);
    stark::PolyArgs a{};
    P2_TRY(pool_alloc(ctx, (pl.num_cols ? pl.num_cols : 1) * n * 8, &d_out.p));
    P2_TRY(stark_blob_alloc(ctx, pl, d_desc, &a.t));
    P2_TRY(pool_alloc(ctx, 2 * (num_z ? num_z : 1) * n_chunks * 8 + 8, &d_sc.p));
    a.trace = trace->d, a.out = d_out.u(), a.n = n, a.num_z = (unsigned)num_z, a.n_chunks = n_chunks;
    a.csum = d_sc.u(), a.carry = a.csum + num_z * n_chunks;
    a.zero_flag = (unsigned *)(d_sc.u() + 2 * (num_z ? num_z : 1) * n_chunks);
    unsigned zero = 0;
    auto body = [&]() -> int {
        P2_HIP(ctx, hipMemcpyAsync(d_desc.p, pl.blob.data(), pl.blob.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        P2_HIP(ctx, hipMemsetAsync(a.zero_flag, 0, 8, ctx->stream));
        if (num_z) {
            {
                ProfScope prof(ctx, "stark_helper_rows");
                P2HOT_LAUNCH(stark::helper_rows_kernel, dim3(cdiv(n, 256), (unsigned)pl.hmap.size()), dim3(256), 0, ctx->stream, a);
                P2_LAUNCH_CHECK(ctx);
            }
            {
                ProfScope prof(ctx, "stark_increments");
                P2HOT_LAUNCH(stark::increments_kernel, dim3(cdiv(n, 256), (unsigned)num_z), dim3(256), 0, ctx->stream, a);
                P2_LAUNCH_CHECK(ctx);
            }
            ProfScope prof(ctx, "stark_scan");
            P2HOT_LAUNCH(stark::scan_totals_kernel, dim3(cdiv(n_chunks, 64), (unsigned)num_z), dim3(64), 0, ctx->stream, a);
            P2_LAUNCH_CHECK(ctx);
            P2HOT_LAUNCH(stark::scan_carries_kernel, dim3((unsigned)num_z), dim3(1024), 0, ctx->stream, a, (n_chunks + 1023) / 1024);
            P2_LAUNCH_CHECK(ctx);
            P2HOT_LAUNCH(stark::scan_emit_kernel, dim3(cdiv(n_chunks, 64), (unsigned)num_z), dim3(64), 0, ctx->stream, a);
            P2_LAUNCH_CHECK(ctx);
        }
        P2_HIP(ctx, hipMemcpyAsync(&zero, a.zero_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
        if (out_host && pl.num_cols) P2_HIP(ctx, hipMemcpyAsync(out_host, d_out.p, pl.num_cols * n * 8, hipMemcpyDeviceToHost, ctx->stream));
        for (unsigned k = 0; k < num_zs_first && zs_first; ++k) P2_TRY(d2h(ctx, zs_first + k, d_out.u() + (first_z_col + k) * n, 8));
        return P2HOT_OK;
    };
    int rc = sync_checked(ctx, body(), what);
    if (rc != P2HOT_OK) return rc;
    if (zero) P2_FAIL(ctx, P2HOT_EINVAL, "%s: Tried to invert zero (a challenge meets a looking, table or combined value; the reference panics in batch_multiplicative_inverse)", what);
    if (out_cols) {
        *out_cols = new p2hot_cols{ctx, d_out.u(), pl.num_cols, log_n, true};
        d_out.p = nullptr;
    }
    return rc;
}

extern "C" int p2hot_stark_lookup_polys(p2hot_ctx *ctx, const p2hot_cols *trace, const p2hot_stark_tables *tables, const p2hot_stark_lookup *lookups,
                                        unsigned num_lookups, const uint64_t *challenges, unsigned num_challenges, unsigned constraint_degree,
                                        uint64_t *out_host, p2hot_cols **out_cols) {
    P2_ENTER(ctx);
    if (out_cols) *out_cols = nullptr;
    if (!trace || trace->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "stark_lookup_polys: null or foreign column set");
    StarkPlan pl;
    P2_TRY(stark_plan(ctx, "stark_lookup_polys", tables, trace->W, lookups, num_lookups, challenges, num_challenges, nullptr, 0, nullptr,
                      constraint_degree, &pl));
    return stark_aux_polys(ctx, "stark_lookup_polys", trace, pl, out_host, out_cols, nullptr, 0, 0);
}

extern "C" int p2hot_stark_ctl_polys(p2hot_ctx *ctx, const p2hot_cols *trace, const p2hot_stark_tables *tables, const p2hot_stark_ctl_z *ctl_zs,
                                     unsigned num_zs, unsigned constraint_degree, uint64_t *out_host, p2hot_cols **out_cols, uint64_t *zs_first) {
    P2_ENTER(ctx);
    if (out_cols) *out_cols = nullptr;
    if (!trace || trace->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "stark_ctl_polys: null or foreign column set");
    StarkPlan pl;
    P2_TRY(stark_plan(ctx, "stark_ctl_polys", tables, trace->W, nullptr, 0, nullptr, 1, ctl_zs, num_zs, nullptr, constraint_degree, &pl));
    return stark_aux_polys(ctx, "stark_ctl_polys", trace, pl, out_host, out_cols, zs_first, pl.num_ctl_helpers, num_zs);
}

// ZeroPolyOnCoset::new(degree_bits, qbits) (field/src/zero_poly_coset.rs:21-34) on the host: out[2 << qbits], the evaluations
// and then their inverses
static int stark_zero_poly_on_coset(p2hot_ctx *ctx, const char *what, unsigned degree_bits, unsigned qbits, u64 *out) {
    const size_t n = (size_t)1 << degree_bits, rate = (size_t)1 << qbits;
    const u64 g_pow_n = gl::pow(gl::COSET_SHIFT, n), v = gl::root_of_unity(qbits);
    for (size_t j = 0; j < rate; ++j) {
        const u64 e = gl::canon(gl::sub(gl::mul(g_pow_n, gl::pow(v, j)), 1));
        if (e == 0) P2_FAIL(ctx, P2HOT_EINVAL, "%s: Z_H vanishes on the coset", what);
        out[j] = e;
        out[rate + j] = gl::inv(e);
    }
    return P2HOT_OK;
}

// 1 / (n (x - 1)) for every point of the quotient coset: the table p2hot_quotient_polys keeps (sizes only)
static int stark_inv_nx1_table(p2hot_ctx *ctx, const char *what, unsigned degree_bits, unsigned qbits, const u64 **out) {
    const unsigned log_nq = degree_bits + qbits;
    const size_t n = (size_t)1 << degree_bits, m = n << qbits;
    const auto inv_key = std::make_tuple(100, log_nq, qbits);
    auto inv_it = ctx->twid_cache.find(inv_key);
    if (inv_it == ctx->twid_cache.end()) {
        u64 *t = nullptr;
        P2_HIP(ctx, hipMalloc((void **)&t, m * 8));
        P2HOT_LAUNCH(plonk::quot_inv_kernel, dim3(cdiv(m, 256)), dim3(256), 0, ctx->stream, t, log_nq, (u64)n % gl::P, ctx->fwd);
        if (hipGetLastError() != hipSuccess) {
            (void)hipFree(t);
            P2_FAIL(ctx, P2HOT_EHIP, "%s: the L_first denominator table could not be launched", what);
        }
        inv_it = ctx->twid_cache.emplace(inv_key, t).first;
    }
    *out = inv_it->second;
    return P2HOT_OK;
}

// p2hot_stark_quotient_polys and p2hot_stark_quotient_polys_air: the STARK's own constraints as the caller's host accumulators
// (constraint_accs, or null) or, with use_air, as a program the interpreter turns into the same [nc][Nq] device buffer
static int stark_quotient_impl(p2hot_ctx *ctx, const char *what, const p2hot_batch *trace, const p2hot_batch *aux, const p2hot_stark_tables *tables,
                               const p2hot_stark_lookup *lookups, unsigned num_lookups, const uint64_t *lookup_challenges,
                               const p2hot_stark_ctl_z *ctl_zs, unsigned num_ctl_zs, const unsigned *ctl_num_helpers, unsigned constraint_degree,
                               const uint64_t *alphas, unsigned num_challenges, const uint64_t *const *constraint_accs, bool use_air,
                               const p2hot_air_program *program, const uint64_t *public_inputs, uint64_t *values_out, p2hot_cols **chunks_out) {
    if (chunks_out) *chunks_out = nullptr;
    if (!trace || !alphas) P2_FAIL(ctx, P2HOT_EINVAL, "%s: null argument", what);
    if (!chunks_out && !values_out) P2_FAIL(ctx, P2HOT_EINVAL, "%s: nothing asked for", what);
    if (trace->ctx != ctx || (aux && aux->ctx != ctx)) P2_FAIL(ctx, P2HOT_EINVAL, "%s: a commitment belongs to another context", what);
    if (aux && (aux->log_n != trace->log_n || aux->rate_bits != trace->rate_bits)) P2_FAIL(ctx, P2HOT_EINVAL, "%s: the commitments differ in degree or rate", what);
    if (trace->hash_n || (aux && aux->hash_n)) P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "%s: KeccakHash commitments are not supported", what);
    StarkPlan pl;
    P2_TRY(stark_plan(ctx, what, tables, trace->W, lookups, num_lookups, lookup_challenges, num_challenges, ctl_zs, num_ctl_zs, ctl_num_helpers,
                      constraint_degree, &pl));
    // qdf = max(1, constraint_degree - 1) with the subtraction saturating, as the chunk size's checked_sub(1).unwrap_or(1): degree 0 is
    // qdf 1 like degree 2 (Stark::quotient_degree_factor, starky/src/stark.rs:87-92, answers 0 there and the reference then computes
    // no quotient at all, prover.rs:508-510); degree 1 was rejected with the descriptors, so the three entry points take the same degrees
    const unsigned qdf = constraint_degree >= 2 ? constraint_degree - 1 : 1, nc = num_challenges;
    unsigned qbits = 0;
    while ((1u << qbits) < qdf) ++qbits;
    if (qbits > trace->rate_bits) P2_FAIL(ctx, P2HOT_EINVAL, "%s: quotient degree 2^%u above the rate 2^%u (prover.rs:517-520)", what, qbits, trace->rate_bits);
    if ((aux ? aux->W : 0) != pl.num_cols)
        P2_FAIL(ctx, P2HOT_EINVAL, "%s: the aux commitment has %zu polynomials, not %zu lookup columns + %zu CTL helpers + %u CTL Zs", what, aux ? aux->W : (size_t)0,
                pl.num_lookup_cols, pl.num_ctl_helpers, num_ctl_zs);
    for (unsigned c = 0; c < nc && constraint_accs; ++c)
        if (!constraint_accs[c]) P2_FAIL(ctx, P2HOT_EINVAL, "%s: constraint_accs[%u] is null", what, c);
    const unsigned degree_bits = trace->log_n, log_nq = degree_bits + qbits, K = pl.K;
    P2_TRY(check_log(ctx, log_nq, what));
    AirPlan airp;
    if (use_air) P2_TRY(air_plan(ctx, what, program, public_inputs, trace->W, alphas, nc, qdf + 1, &airp));
    const bool run_air = use_air && !airp.empty(), have_accs = constraint_accs || run_air;
    const size_t n = (size_t)1 << degree_bits, m = n << qbits, rate = (size_t)1 << qbits;
    // ZeroPolyOnCoset::new(degree_bits, qbits) and the alpha powers, on the host
    const size_t n_small = 2 * rate + (size_t)nc * (K + 1);
    std::vector<u64> small(n_small);
    P2_TRY(stark_zero_poly_on_coset(ctx, what, degree_bits, qbits, small.data()));
    for (unsigned a = 0; a < nc; ++a) {  // term t carries alpha^(K-1-t); the caller's accumulator alpha^K
        u64 *ap = small.data() + 2 * rate + (size_t)a * (K + 1), pw = 1;
        for (unsigned t = 0; t < K; ++t, pw = gl::mul(pw, alphas[a])) ap[K - 1 - t] = gl::canon(pw);
        ap[K] = gl::canon(pw);
    }
    PoolBuf d_work(ctx), d_small(ctx), d_desc(ctx), d_acc(ctx), d_air(ctx);
    stark::TermArgs q{};
    air::Args qa{};
    P2_TRY(pool_alloc(ctx, (size_t)nc * m * 8 + 8, &d_work.p));
    P2_TRY(pool_alloc(ctx, n_small * 8, &d_small.p));
    P2_TRY(stark_blob_alloc(ctx, pl, d_desc, &q.t));
    if (have_accs) P2_TRY(pool_alloc(ctx, (size_t)nc * m * 8, &d_acc.p));
    if (run_air) P2_TRY(air_blob_alloc(ctx, airp, d_air, &qa));
    P2_TRY(stark_inv_nx1_table(ctx, what, degree_bits, qbits, &q.inv_nx1));
    q.trace = trace->d_lde, q.trace_stride = trace->col_stride_lde();
    q.aux = aux ? aux->d_lde : nullptr, q.aux_stride = aux ? aux->col_stride_lde() : 0;
    q.zh = d_small.u(), q.apow = d_small.u() + 2 * rate;
    q.accs = have_accs ? d_acc.u() : nullptr, q.out = d_work.u();
    q.num_z = (unsigned)pl.zs.size(), q.K = K, q.chunk = pl.chunk, q.log_nq = log_nq, q.qbits = qbits;
    q.last = gl::inv(gl::root_of_unity(degree_bits));  // prover.rs:538
    q.roots = ctx->fwd;
    qa.trace = q.trace, qa.stride = q.trace_stride, qa.zh = q.zh, qa.inv_nx1 = q.inv_nx1, qa.out = d_acc.u();
    qa.log_nq = log_nq, qa.qbits = qbits, qa.last = q.last, qa.roots = ctx->fwd;
    auto body = [&]() -> int {
        P2_HIP(ctx, hipMemcpyAsync(d_small.p, small.data(), small.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        P2_HIP(ctx, hipMemcpyAsync(d_desc.p, pl.blob.data(), pl.blob.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        for (unsigned c = 0; c < nc && constraint_accs; ++c)
            P2_HIP(ctx, hipMemcpyAsync(d_acc.u() + (size_t)c * m, constraint_accs[c], m * 8, hipMemcpyHostToDevice, ctx->stream));
        if (run_air) P2_TRY(air_enqueue(ctx, airp, d_air, qa, nc));
        ProfScope prof(ctx, "stark_aux_terms");
        const dim3 grid(cdiv(m, 256)), block(256);
        switch (nc) {
            case 1: P2HOT_LAUNCH((stark::aux_terms_kernel<1>), grid, block, 0, ctx->stream, q); break;
            case 2: P2HOT_LAUNCH((stark::aux_terms_kernel<2>), grid, block, 0, ctx->stream, q); break;
            case 3: P2HOT_LAUNCH((stark::aux_terms_kernel<3>), grid, block, 0, ctx->stream, q); break;
            default: P2HOT_LAUNCH((stark::aux_terms_kernel<4>), grid, block, 0, ctx->stream, q); break;
        }
        P2_LAUNCH_CHECK(ctx);
        if (values_out) P2_HIP(ctx, hipMemcpyAsync(values_out, d_work.p, (size_t)nc * m * 8, hipMemcpyDeviceToHost, ctx->stream));
        return P2HOT_OK;
    };
    int rc = body();
    if (rc != P2HOT_OK || !chunks_out) return sync_checked(ctx, rc, what);
    return quotient_chunks_core(ctx, d_work, nc, degree_bits, qbits, qdf, what, chunks_out);
}

extern "C" int p2hot_stark_quotient_polys(p2hot_ctx *ctx, const p2hot_batch *trace, const p2hot_batch *aux, const p2hot_stark_tables *tables,
                                          const p2hot_stark_lookup *lookups, unsigned num_lookups, const uint64_t *lookup_challenges,
                                          const p2hot_stark_ctl_z *ctl_zs, unsigned num_ctl_zs, const unsigned *ctl_num_helpers,
                                          unsigned constraint_degree, const uint64_t *alphas, unsigned num_challenges,
                                          const uint64_t *const *constraint_accs, uint64_t *values_out, p2hot_cols **chunks_out) {
    P2_ENTER(ctx);
    return stark_quotient_impl(ctx, "stark_quotient_polys", trace, aux, tables, lookups, num_lookups, lookup_challenges, ctl_zs, num_ctl_zs,
                               ctl_num_helpers, constraint_degree, alphas, num_challenges, constraint_accs, false, nullptr, nullptr, values_out, chunks_out);
}

extern "C" int p2hot_stark_quotient_polys_air(p2hot_ctx *ctx, const p2hot_batch *trace, const p2hot_batch *aux, const p2hot_stark_tables *tables,
                                              const p2hot_stark_lookup *lookups, unsigned num_lookups, const uint64_t *lookup_challenges,
                                              const p2hot_stark_ctl_z *ctl_zs, unsigned num_ctl_zs, const unsigned *ctl_num_helpers,
                                              unsigned constraint_degree, const uint64_t *alphas, unsigned num_challenges,
                                              const p2hot_air_program *program, const uint64_t *public_inputs, uint64_t *values_out,
                                              p2hot_cols **chunks_out) {
    P2_ENTER(ctx);
    return stark_quotient_impl(ctx, "stark_quotient_polys_air", trace, aux, tables, lookups, num_lookups, lookup_challenges, ctl_zs, num_ctl_zs,
                               ctl_num_helpers, constraint_degree, alphas, num_challenges, nullptr, true, program, public_inputs, values_out, chunks_out);
}

extern "C" int p2hot_stark_constraint_accs(p2hot_ctx *ctx, const p2hot_batch *trace, const p2hot_air_program *program, const uint64_t *public_inputs,
                                           unsigned constraint_degree, const uint64_t *alphas, unsigned num_challenges, uint64_t *accs_out) {
    P2_ENTER(ctx);
    const char *what = "stark_constraint_accs";
    if (!trace || !alphas || !accs_out) P2_FAIL(ctx, P2HOT_EINVAL, "%s: null argument", what);
    if (trace->ctx != ctx) P2_FAIL(ctx, P2HOT_EINVAL, "%s: the commitment belongs to another context", what);
    if (trace->hash_n) P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "%s: KeccakHash commitments are not supported", what);
    const unsigned nc = num_challenges;
    if (nc == 0 || nc > 4) P2_FAIL(ctx, P2HOT_EINVAL, "%s: %u challenges (1..4)", what, nc);
    // the degrees p2hot_stark_quotient_polys takes: 1 is rejected there with the descriptors, 0 is qdf 1
    if (constraint_degree == 1) P2_FAIL(ctx, P2HOT_EINVAL, "%s: constraint_degree 1 (chunks of constraint_degree - 1 = 0 columns)", what);
    const unsigned qdf = constraint_degree >= 2 ? constraint_degree - 1 : 1;
    unsigned qbits = 0;
    while ((1u << qbits) < qdf) ++qbits;
    if (qbits > trace->rate_bits) P2_FAIL(ctx, P2HOT_EINVAL, "%s: quotient degree 2^%u above the rate 2^%u (prover.rs:517-520)", what, qbits, trace->rate_bits);
    const unsigned degree_bits = trace->log_n, log_nq = degree_bits + qbits;
    P2_TRY(check_log(ctx, log_nq, what));
    AirPlan airp;
    P2_TRY(air_plan(ctx, what, program, public_inputs, trace->W, alphas, nc, qdf + 1, &airp));
    const size_t m = (size_t)1 << log_nq, rate = (size_t)1 << qbits;
    if (airp.empty()) {  // no constraints: the consumer's accumulators stay zero
        std::fill(accs_out, accs_out + (size_t)nc * m, (uint64_t)0);
        return P2HOT_OK;
    }
    std::vector<u64> zh(2 * rate);
    P2_TRY(stark_zero_poly_on_coset(ctx, what, degree_bits, qbits, zh.data()));
    PoolBuf d_acc(ctx), d_zh(ctx), d_air(ctx);
    air::Args qa{};
    P2_TRY(pool_alloc(ctx, (size_t)nc * m * 8, &d_acc.p));
    P2_TRY(pool_alloc(ctx, zh.size() * 8, &d_zh.p));
    P2_TRY(air_blob_alloc(ctx, airp, d_air, &qa));
    P2_TRY(stark_inv_nx1_table(ctx, what, degree_bits, qbits, &qa.inv_nx1));
    qa.trace = trace->d_lde, qa.stride = trace->col_stride_lde(), qa.zh = d_zh.u(), qa.out = d_acc.u();
    qa.log_nq = log_nq, qa.qbits = qbits, qa.last = gl::inv(gl::root_of_unity(degree_bits)), qa.roots = ctx->fwd;
    auto body = [&]() -> int {
        P2_HIP(ctx, hipMemcpyAsync(d_zh.p, zh.data(), zh.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        P2_TRY(air_enqueue(ctx, airp, d_air, qa, nc));
        P2_HIP(ctx, hipMemcpyAsync(accs_out, d_acc.p, (size_t)nc * m * 8, hipMemcpyDeviceToHost, ctx->stream));
        return P2HOT_OK;
    };
    return sync_checked(ctx, body(), what);
}
