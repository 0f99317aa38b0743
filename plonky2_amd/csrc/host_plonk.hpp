// host_plonk.hpp -- the MIDDLE of a proof in the host-pointer layer of libp2hot: what lies between the wires commitment and the
// opening proof.  Included by p2hot.hip behind host_prover.hpp (one TU), whose call guard, handles and commitments it uses.
//
// Reference call sites this layer stands behind:
//   all_wires_permutation_partial_products         plonk/prover.rs:356-449               p2hot_partial_products
//   compute_lookup_polys                           plonk/prover.rs:451-605               p2hot_lookup_polys
//   compute_quotient_polys                         plonk/prover.rs:609-815               p2hot_quotient_polys, its _lookup / _gates / _gate_programs forms
//   quotient coset_ifft + chunks                   plonk/prover.rs:274-289, :810-815     p2hot_quotient_chunks
//   evaluate_gate_constraints_base_batch           plonk/vanishing_poly.rs:702-728       p2hot_gate_sums
// and the M-forms of the first and the third for M witnesses of one circuit.  A single-proof entry point and its M-form share their
// host planning and launch helpers (PPPlan / pp_launch in p2hot.hip; QuotShape, the quot_* tables, quotient_perm_launch and
// gates_launch here); they differ in their validation messages, the per-proof device table and the kernel pair the table selects.
#pragma once

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

// ------------------------------------------------------------------ the quotient's sizes and tables, for one proof or M
// what follows from (degree, rate, challenges, factor, routed wires) alone: the same for every proof of an M-form call
struct QuotShape {
    unsigned nc, qdf, qbits, num_chunks, num_prods, degree_bits, log_nq;
    size_t n, m, rate, keep;  // rows, points of the quotient coset, m / n, coefficients trim_to_len keeps
};

// the shape and the checks that do not look at a particular proof; `ref`: a commitment of the circuit's degree and rate
static int quot_shape(p2hot_ctx *ctx, const char *what, const p2hot_batch *ref, unsigned num_challenges, unsigned quotient_degree_factor,
                      unsigned num_routed, QuotShape *s) {
    if (num_challenges == 0 || num_challenges > 4) P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "%s: %u challenges (1..4 supported; plonky2's configs use 2)", what, num_challenges);
    if (quotient_degree_factor < 2 || num_routed == 0) P2_FAIL(ctx, P2HOT_EINVAL, "%s: bad quotient degree factor or no routed wires", what);
    s->nc = num_challenges, s->qdf = quotient_degree_factor, s->qbits = 0;
    while ((1u << s->qbits) < quotient_degree_factor) ++s->qbits;  // log2_ceil (circuit_data.rs quotient_degree_bits)
    // "Having constraints of degree higher than the rate is not supported yet." (prover.rs:632-636)
    if (s->qbits > ref->rate_bits) P2_FAIL(ctx, P2HOT_EINVAL, "%s: quotient degree 2^%u above the rate 2^%u (prover.rs:632-636)", what, s->qbits, ref->rate_bits);
    s->degree_bits = ref->log_n, s->log_nq = s->degree_bits + s->qbits;
    P2_TRY(check_log(ctx, s->log_nq, what));
    s->num_chunks = (num_routed + quotient_degree_factor - 1) / quotient_degree_factor, s->num_prods = s->num_chunks - 1;
    s->n = (size_t)1 << s->degree_bits, s->m = s->n << s->qbits, s->rate = (size_t)1 << s->qbits, s->keep = s->n * quotient_degree_factor;
    return P2HOT_OK;
}

// row [nc][num_routed] of one proof: beta_c * k_j
static void quot_bk_table(u64 *bk, const uint64_t *betas, const uint64_t *k_is, unsigned nc, unsigned num_routed) {
    for (unsigned c = 0; c < nc; ++c)
        for (unsigned j = 0; j < num_routed; ++j) bk[(size_t)c * num_routed + j] = gl::canon(gl::mul(betas[c], k_is[j]));
}

// zh [2 << qbits]: ZeroPolyOnCoset::new(degree_bits, qbits) (field/src/zero_poly_coset.rs:21-34), the values then their inverses
static int quot_zh_table(p2hot_ctx *ctx, const char *what, const QuotShape &s, u64 *zh) {
    const u64 g_pow_n = gl::pow(gl::COSET_SHIFT, s.n), v = gl::root_of_unity(s.qbits);
    for (size_t j = 0; j < s.rate; ++j) {
        const u64 e = gl::canon(gl::sub(gl::mul(g_pow_n, gl::pow(v, j)), 1));
        if (e == 0) P2_FAIL(ctx, P2HOT_EINVAL, "%s: Z_H vanishes on the coset", what);
        zh[j] = e;
        zh[s.rate + j] = gl::inv(e);
    }
    return P2HOT_OK;
}

// 1 / (n (x - 1)) for every point of the quotient coset: sizes only, kept by the context
static int quot_inv_table(p2hot_ctx *ctx, const char *what, const QuotShape &s, const u64 **table) {
    const auto inv_key = std::make_tuple(100, s.log_nq, s.qbits);
    auto inv_it = ctx->twid_cache.find(inv_key);
    if (inv_it == ctx->twid_cache.end()) {
        u64 *t = nullptr;
        P2_HIP(ctx, hipMalloc((void **)&t, s.m * 8));
        P2HOT_LAUNCH(plonk::quot_inv_kernel, dim3(cdiv(s.m, 256)), dim3(256), 0, ctx->stream, t, s.log_nq, (u64)s.n % gl::P, ctx->fwd);
        if (hipGetLastError() != hipSuccess) {
            (void)hipFree(t);
            P2_FAIL(ctx, P2HOT_EHIP, "%s: the L_0 denominator table could not be launched", what);
        }
        inv_it = ctx->twid_cache.emplace(inv_key, t).first;
    }
    *table = inv_it->second;
    return P2HOT_OK;
}

// one proof's challenges and alpha tables into a plonk::QuotArgs (the kernel's arguments) or a plonk::ManyProof (its table entry)
template <class T>
static void quot_challenges(T &t, const QuotShape &s, const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas) {
    const u64 K = (u64)s.nc + (u64)s.nc * s.num_chunks;
    for (unsigned a = 0; a < s.nc; ++a) {
        t.betas[a] = betas[a], t.gammas[a] = gl::canon(gammas[a]), t.alphas[a] = alphas[a];
        t.alpha_k[a] = gl::pow(alphas[a], K);
        for (unsigned c = 0; c < s.nc; ++c) t.base[a][c] = gl::pow(alphas[a], (u64)s.nc + (u64)c * s.num_chunks);
    }
}

// ------------------------------------------------------------------ quotient polynomials -> chunks (plonk/prover.rs:274-289, :810-815)
// the tail the single-proof quotient entry points share: d_work holds num_challenges polynomials' VALUES on g*H of size m = n << qbits
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

// the M-form's tail: d_work holds the values of M * nc polynomials (one flag word per proof behind them); coset_ifft on all of them,
// trim_to_len with one divisibility flag per proof, and the chunks straight into the interleaved layout of d_chunks, which becomes
// *chunks_out.  Synchronises the call.
static int quotient_chunks_many(p2hot_ctx *ctx, PoolBuf &d_work, PoolBuf &d_chunks, size_t M, const QuotShape &s, const char *what,
                                p2hot_cols **chunks_out) {
    unsigned *flags = (unsigned *)(d_work.u() + M * s.nc * s.m);
    std::vector<unsigned> nonzero(M, 0);
    auto body = [&]() -> int {
        P2_TRY(p2hot_coset_ifft_dev(ctx, d_work.u(), M * s.nc, s.m, s.log_nq, gl::COSET_SHIFT));  // values.coset_ifft(F::coset_shift())
        P2_HIP(ctx, hipMemsetAsync(flags, 0, M * 8, ctx->stream));
        if (s.keep < s.m) {
            P2HOT_LAUNCH(plonk::any_nonzero_many_kernel, dim3(cdiv(s.m - s.keep, 256), s.nc, (unsigned)M), dim3(256), 0, ctx->stream,
                         (const u64 *)d_work.u(), s.m, s.keep, flags);
            P2_LAUNCH_CHECK(ctx);
        }
        P2HOT_LAUNCH(plonk::chunks_interleave_kernel, dim3(cdiv(s.n, 256), s.nc * s.qdf, (unsigned)M), dim3(256), 0, ctx->stream,
                     (const u64 *)d_work.u(), s.m, s.n, s.qdf, s.nc, d_chunks.u());
        P2_LAUNCH_CHECK(ctx);
        return d2h(ctx, nonzero.data(), flags, M * 4);
    };
    int rc = sync_checked(ctx, body(), what);
    if (rc != P2HOT_OK) return rc;
    for (size_t j = 0; j < M; ++j)
        if (nonzero[j]) P2_FAIL(ctx, P2HOT_EINVAL, "Quotient has failed, the vanishing polynomial is not divisible by Z_H (proof %zu)", j);
    *chunks_out = new p2hot_cols{ctx, d_chunks.u(), (size_t)s.nc * s.qdf * M, s.degree_bits, true};
    d_chunks.p = nullptr;
    return P2HOT_OK;
}

extern "C" int p2hot_quotient_chunks(p2hot_ctx *ctx,const uint64_t *const *quotient_values, unsigned num_challenges,
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
#define P2_GATES_LAUNCH_NC(kernel, ...)                                                                    \
    switch (nc) {                                                                                          \
        case 1: P2HOT_LAUNCH((gates::kernel<1>), grid, block, 0, ctx->stream, __VA_ARGS__); break;         \
        case 2: P2HOT_LAUNCH((gates::kernel<2>), grid, block, 0, ctx->stream, __VA_ARGS__); break;         \
        case 3: P2HOT_LAUNCH((gates::kernel<3>), grid, block, 0, ctx->stream, __VA_ARGS__); break;         \
        default: P2HOT_LAUNCH((gates::kernel<4>), grid, block, 0, ctx->stream, __VA_ARGS__); break;        \
    }
#define P2_GATES_LAUNCH(name, args)                                        \
    do {                                                                   \
        if (d_many) P2_GATES_LAUNCH_NC(name##_many_kernel, args, d_many)   \
        else P2_GATES_LAUNCH_NC(name##_kernel, args)                       \
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
    for (const bool mds : {true, false})  // every PoseidonMdsGate, then every PoseidonGate
        for (unsigned k = 0; k < gs->num_gates; ++k) {
            if (gs->gates[k].kind != (mds ? (unsigned)P2HOT_GATE_POSEIDON_MDS : (unsigned)P2HOT_GATE_POSEIDON)) continue;
            gates::PoseidonArgs pa{};
            pa.wires = a.wires, pa.wires_stride = a.wires_stride, pa.consts = a.consts, pa.consts_stride = a.consts_stride;
            pa.apow = d_apow, pa.apow_stride = apow_stride, pa.out = d_out, pa.log_nq = log_nq, pa.num_selectors = gs->num_selectors;
            pa.gate = gs->gates[k];
            ProfScope prof(ctx, mds ? "gates_poseidon_mds" : "gates_poseidon");
            if (mds) P2_GATES_LAUNCH(mds_gate, pa);
            else P2_GATES_LAUNCH(poseidon_gate, pa);
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

// ------------------------------------------------------------------ the quotient's own launches
// (they stand behind the gates' and in this order because that is the order in which the kernel templates are instantiated)
// the lookup argument's terms into the gate-sum buffer (lookup::lookup_terms_kernel)
static int lookup_terms_launch(p2hot_ctx *ctx, const lookup::TermArgs &lt, unsigned nc) {
    ProfScope prof(ctx, "quotient_lookup");
    const dim3 grid(cdiv((size_t)1 << lt.log_nq, 256)), block(256);
    switch (nc) {
        case 1: P2HOT_LAUNCH((lookup::lookup_terms_kernel<1>), grid, block, 0, ctx->stream, lt); break;
        case 2: P2HOT_LAUNCH((lookup::lookup_terms_kernel<2>), grid, block, 0, ctx->stream, lt); break;
        case 3: P2HOT_LAUNCH((lookup::lookup_terms_kernel<3>), grid, block, 0, ctx->stream, lt); break;
        default: P2HOT_LAUNCH((lookup::lookup_terms_kernel<4>), grid, block, 0, ctx->stream, lt); break;
    }
    P2_LAUNCH_CHECK(ctx);
    return P2HOT_OK;
}

// the permutation terms over Z_H for M proofs, one grid row each.  d_tab == NULL: one proof, everything in `q`; else the M-form
// kernel, which takes the per-proof fields from d_tab[blockIdx.y]
#define P2_QUOT_PERM_LAUNCH(kernel, ...)                                                                                \
    do {                                                                                                                \
        if (nc == 2 && qdf == 8) { /* every plonky2 config (circuit_data.rs:101-119): the pipelined instantiation */    \
            P2HOT_LAUNCH((plonk::kernel<2, 8>), grid, block, 0, ctx->stream, __VA_ARGS__);                              \
        } else {                                                                                                        \
            switch (nc) {                                                                                               \
                case 1: P2HOT_LAUNCH((plonk::kernel<1, 0>), grid, block, 0, ctx->stream, __VA_ARGS__); break;           \
                case 2: P2HOT_LAUNCH((plonk::kernel<2, 0>), grid, block, 0, ctx->stream, __VA_ARGS__); break;           \
                case 3: P2HOT_LAUNCH((plonk::kernel<3, 0>), grid, block, 0, ctx->stream, __VA_ARGS__); break;           \
                default: P2HOT_LAUNCH((plonk::kernel<4, 0>), grid, block, 0, ctx->stream, __VA_ARGS__); break;          \
            }                                                                                                           \
        }                                                                                                               \
    } while (0)
static int quotient_perm_launch(p2hot_ctx *ctx, const plonk::QuotArgs &q, const plonk::ManyProof *d_tab, size_t M, unsigned nc, unsigned qdf) {
    const dim3 grid(cdiv((size_t)1 << q.log_nq, 256), (unsigned)M), block(256);
    if (!d_tab)
        P2_QUOT_PERM_LAUNCH(quotient_perm_kernel, q);
    else
        P2_QUOT_PERM_LAUNCH(quotient_perm_many_kernel, q, d_tab);
    P2_LAUNCH_CHECK(ctx);
    return P2HOT_OK;
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
    QuotShape s;
    P2_TRY(quot_shape(ctx, "quotient_polys", wires, num_challenges, quotient_degree_factor, num_routed, &s));
    const unsigned qbits = s.qbits, log_nq = s.log_nq, num_prods = s.num_prods;
    const size_t m = s.m, rate = s.rate;
    if (wires->W < num_routed || constants_sigmas->W < sigmas_first_col + num_routed || zs_partial_products->W < (size_t)num_challenges * (1 + num_prods))
        P2_FAIL(ctx, P2HOT_EINVAL, "quotient_polys: a commitment is narrower than the permutation argument needs");
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
    // small: beta_c k_j [nc][num_routed] | Z_H and inverses [2 rate] | lookup alpha powers | LUT evaluations | gate alpha powers, on the host
    std::vector<u64> small(nbk + 2 * rate + n_apow + n_evals + n_gpow);
    if (with_gates) gates_alpha_powers(small.data() + nbk + 2 * rate + n_apow + n_evals, alphas, num_challenges, gs_stride);
    quot_bk_table(small.data(), betas, k_is, num_challenges, num_routed);
    P2_TRY(quot_zh_table(ctx, "quotient_polys", s, small.data() + nbk));
    plonk::QuotArgs q{};
    P2_TRY(quot_inv_table(ctx, "quotient_polys", s, &q.inv_nx1));
    q.wires = wires->d_lde, q.wires_stride = wires->col_stride_lde();
    q.sigmas = constants_sigmas->d_lde + sigmas_first_col * constants_sigmas->col_stride_lde(), q.sigmas_stride = constants_sigmas->col_stride_lde();
    q.zs = zs_partial_products->d_lde, q.zs_stride = zs_partial_products->col_stride_lde();
    q.bk = d_small.u(), q.zh = d_small.u() + nbk;
    q.gate_sums = gate_sums || lk || with_gates ? d_gate.u() : nullptr;
    q.out = d_work.u();
    q.num_routed = num_routed, q.degree = quotient_degree_factor, q.num_chunks = s.num_chunks, q.log_nq = log_nq, q.qbits = qbits;
    quot_challenges(q, s, betas, gammas, alphas);
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
        if (lk) P2_TRY(lookup_terms_launch(ctx, lt, num_challenges));
        ProfScope prof(ctx, "quotient_perm");
        P2_TRY(quotient_perm_launch(ctx, q, nullptr, 1, num_challenges, quotient_degree_factor));
        if (values_out) P2_HIP(ctx, hipMemcpyAsync(values_out, d_work.p, (size_t)num_challenges * m * 8, hipMemcpyDeviceToHost, ctx->stream));
        return P2HOT_OK;
    };
    int rc = body();
    if (rc != P2HOT_OK || !chunks_out) return sync_checked(ctx, rc, "quotient_polys");
    return quotient_chunks_core(ctx, d_work, num_challenges, s.degree_bits, qbits, quotient_degree_factor, "quotient_polys", chunks_out);
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
// p2hot_commit_many and p2hot_prove_openings_many batch the two ends of M recursion-size proofs; four calls batch what lies between:
// partial products and Zs and the quotient with its gate constraints here, the commitment of an interleaved device column set
// (p2hot_commit_cols_many) and the OpeningSet (p2hot_eval_openings_many) beside their single-proof forms in host_prover.hpp.  Sigmas,
// constants, selectors, the gate set and k_is are shared; wires, challenges and the public-inputs hash are per proof and reach the
// kernels through a device table indexed by blockIdx.y (plonk::ManyProof, gates::ManyGate).  Every argument is checked before the
// first enqueue, a per-proof message names the proof, and each call synchronises once.

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
    PPPlan pl{M, num_routed, degree, log_n, nc};
    const size_t n = pl.n, rows = (size_t)nc * (pl.num_prods + 1);
    const size_t tab_words = M * sizeof(plonk::ManyProof) / 8;  // small: k_is | the per-proof table
    PoolBuf d_out(ctx), d_vals(ctx), d_scr(ctx), d_small(ctx);
    P2_TRY(pool_alloc(ctx, rows * M * n * 8, &d_out.p));
    P2_TRY(pool_alloc(ctx, M * num_routed * n * 8, &d_vals.p));
    P2_TRY(pool_alloc(ctx, pl.scratch_words() * 8, &d_scr.p));
    P2_TRY(pool_alloc(ctx, (num_routed + tab_words) * 8, &d_small.p));
    pl.carve(d_scr.u());
    std::vector<u64> small(num_routed + tab_words);
    for (unsigned j = 0; j < num_routed; ++j) small[j] = gl::canon(k_is[j]);
    plonk::ManyProof *tab = reinterpret_cast<plonk::ManyProof *>(small.data() + num_routed);
    for (size_t j = 0; j < M; ++j) {
        plonk::ManyProof t{};
        t.coef_off = many_words_between(wires[j]->d_coef, wires[0]->d_coef), t.coef_stride = wires[j]->col_stride_coef();
        for (unsigned c = 0; c < nc; ++c) t.betas[c] = gl::canon(betas[j * nc + c]), t.gammas[c] = gl::canon(gammas[j * nc + c]);
        tab[j] = t;
    }
    const plonk::ManyProof *d_tab = reinterpret_cast<const plonk::ManyProof *>(d_small.u() + num_routed);
    std::vector<unsigned> zero(M, 0);
    auto body = [&]() -> int {
        P2_HIP(ctx, hipMemcpyAsync(d_small.p, small.data(), small.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        P2_HIP(ctx, hipMemsetAsync(pl.flags, 0, M * 8, ctx->stream));
        // the routed wires' values on H: a forward NTT of a copy of every proof's coefficients (p2hot_batch_subgroup_values' route)
        P2HOT_LAUNCH(plonk::many_gather_coeffs_kernel, dim3(cdiv(n, 256), num_routed, (unsigned)M), dim3(256), 0, ctx->stream, (const u64 *)wires[0]->d_coef, d_tab,
                     wires_first_col, n, d_vals.u());
        P2_LAUNCH_CHECK(ctx);
        P2_TRY(p2hot_fft_dev(ctx, d_vals.u(), M * num_routed, n, log_n));
        P2HOT_LAUNCH(ntt::canon_kernel, dim3(cdiv(M * num_routed * n, 256)), dim3(256), 0, ctx->stream, d_vals.u(), M * num_routed * n);
        P2_LAUNCH_CHECK(ctx);
        ProfScope ps(ctx, "partial_products_many");
        // the output is interleaved: column e of proof m is column e * M + m, so a column of the M proofs is M * n words
        P2_TRY(pp_launch(ctx, pl, pp_args(ctx, pl, d_vals.u(), n, sigmas->d + sigmas_first_col * n, n, d_small.u(), nullptr, nullptr, d_out.u(), M * n),
                         d_out.u(), M * n, d_tab));
        if (out_host)  // [M][rows][n] <- [rows][M][n]: one strided copy per proof
            for (size_t j = 0; j < M; ++j) P2_TRY(d2h_2d(ctx, out_host + j * rows * n, n * 8, d_out.u() + j * n, M * n * 8, n * 8, rows));
        P2_TRY(d2h(ctx, zero.data(), pl.flags, M * 4));
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
    QuotShape s;
    P2_TRY(quot_shape(ctx, what, constants_sigmas, num_challenges, quotient_degree_factor, num_routed, &s));
    const unsigned nc = s.nc, log_nq = s.log_nq;
    const size_t m = s.m, rate = s.rate;
    P2_TRY(many_check(ctx, what, "wires", wires, M, constants_sigmas, num_routed));
    P2_TRY(many_check(ctx, what, "zs_partial_products", zs_partial_products, M, constants_sigmas, (size_t)nc * (1 + s.num_prods)));
    for (size_t j = 0; j < M; ++j)
        if (gs && wires[j]->col_stride_lde() >> 32)
            P2_FAIL(ctx, P2HOT_EINVAL, "%s: proof %zu: a wires column stride of %zu words (the gate kernels' M-form takes less than 2^32)", what, j,
                    wires[j]->col_stride_lde());
    for (size_t j = 1; j < M; ++j)
        if (wires[j]->W != wires[0]->W) P2_FAIL(ctx, P2HOT_EINVAL, "%s: proof %zu: %zu wires, proof 0 has %zu (one circuit)", what, j, wires[j]->W, wires[0]->W);
    if (constants_sigmas->W < sigmas_first_col + num_routed) P2_FAIL(ctx, P2HOT_EINVAL, "%s: the constants_sigmas commitment is narrower than the permutation argument needs", what);
    if (M > 65535 || M * nc * quotient_degree_factor > 65535)
        P2_FAIL(ctx, P2HOT_EINVAL, "%s: W * M = %zu polynomials exceed one launch (65535)", what, M * nc * quotient_degree_factor);
    unsigned gs_stride = 0;
    if (gs) P2_TRY(gates_validate(ctx, gs, wires[0], constants_sigmas, sigmas_first_col, quotient_degree_factor, what, &gs_stride));
    // small: beta_c k_j [M][nc][num_routed] | Z_H and inverses [2 rate] | gate alpha powers [M][nc][gs_stride] | ManyProof [M] | ManyGate [M]
    const size_t nbk = M * nc * num_routed, n_gpow = M * nc * gs_stride, w_tab = M * sizeof(plonk::ManyProof) / 8, w_gtab = M * sizeof(gates::ManyGate) / 8;
    const size_t o_zh = nbk, o_gpow = o_zh + 2 * rate, o_tab = o_gpow + n_gpow, o_gtab = o_tab + w_tab;
    std::vector<u64> small(o_gtab + w_gtab);
    P2_TRY(quot_zh_table(ctx, what, s, small.data() + o_zh));
    plonk::ManyProof *tab = reinterpret_cast<plonk::ManyProof *>(small.data() + o_tab);
    gates::ManyGate *gtab = reinterpret_cast<gates::ManyGate *>(small.data() + o_gtab);
    for (size_t j = 0; j < M; ++j) {
        const uint64_t *be = betas + j * nc, *ga = gammas + j * nc, *al = alphas + j * nc;
        quot_bk_table(small.data() + j * nc * num_routed, be, k_is, nc, num_routed);
        if (gs) gates_alpha_powers(small.data() + o_gpow + j * nc * gs_stride, al, nc, gs_stride);
        plonk::ManyProof t{};
        t.wires_off = many_words_between(wires[j]->d_lde, wires[0]->d_lde), t.wires_stride = wires[j]->col_stride_lde();
        t.zs_off = many_words_between(zs_partial_products[j]->d_lde, zs_partial_products[0]->d_lde), t.zs_stride = zs_partial_products[j]->col_stride_lde();
        quot_challenges(t, s, be, ga, al);
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
    if (chunks_out) P2_TRY(pool_alloc(ctx, M * nc * quotient_degree_factor * s.n * 8, &d_chunks.p));
    plonk::QuotArgs q{};  // the shared fields and proof 0's matrices; the kernel takes the rest from the table
    P2_TRY(quot_inv_table(ctx, what, s, &q.inv_nx1));
    q.wires = wires[0]->d_lde, q.zs = zs_partial_products[0]->d_lde;
    q.sigmas = constants_sigmas->d_lde + sigmas_first_col * constants_sigmas->col_stride_lde(), q.sigmas_stride = constants_sigmas->col_stride_lde();
    q.bk = d_small.u(), q.zh = d_small.u() + o_zh;
    q.gate_sums = gs ? d_gate.u() : nullptr;
    q.out = d_work.u();
    q.num_routed = num_routed, q.degree = quotient_degree_factor, q.num_chunks = s.num_chunks, q.log_nq = log_nq, q.qbits = s.qbits;
    q.roots = ctx->fwd;
    const plonk::ManyProof *d_tab = reinterpret_cast<const plonk::ManyProof *>(d_small.u() + o_tab);
    const gates::ManyGate *d_gtab = reinterpret_cast<const gates::ManyGate *>(d_small.u() + o_gtab);
    auto body = [&]() -> int {
        P2_HIP(ctx, hipMemcpyAsync(d_small.p, small.data(), small.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        if (gs) {
            P2_HIP(ctx, hipMemsetAsync(d_gate.p, 0, M * nc * m * 8, ctx->stream));
            P2_TRY(gates_launch(ctx, gs, wires[0], constants_sigmas, d_small.u() + o_gpow, gs_stride, d_gate.u(), log_nq, nc, d_gtab, M));
        }
        {
            ProfScope prof(ctx, "quotient_perm_many");
            P2_TRY(quotient_perm_launch(ctx, q, d_tab, M, nc, quotient_degree_factor));
        }
        if (values_out) P2_HIP(ctx, hipMemcpyAsync(values_out, d_work.p, M * nc * m * 8, hipMemcpyDeviceToHost, ctx->stream));
        return P2HOT_OK;
    };
    int rc = body();
    if (rc != P2HOT_OK || !chunks_out) return sync_checked(ctx, rc, what);
    return quotient_chunks_many(ctx, d_work, d_chunks, M, s, what, chunks_out);
}
