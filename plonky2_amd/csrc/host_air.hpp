// host_air.hpp -- the host side of the constraint-program interpreter (include/p2hot.h, "constraint program"; kernel in air.hpp):
// every check of a program, its device image, the launch.  Included in p2hot.hip before host_stark.hpp, whose entry points
// p2hot_stark_constraint_accs and p2hot_stark_quotient_polys_air stand in front of it.
#pragma once

namespace {
// a checked program: canonical constants, public inputs and alphas, and where they lie in one device block
struct AirPlan {
    std::vector<p2hot_air_insn> insns;
    std::vector<u64> constants, publics, alphas;
    unsigned num_temps = 0;
    std::vector<u64> blob;  // host image of the device block (outlives the asynchronous copy)
    bool empty() const { return insns.empty(); }
};
}  // namespace

extern "C" unsigned p2hot_air_max_temps(void) { return air::MAX_TEMPS; }

// every check of the program, before anything is enqueued (include/p2hot.h lists them); max_degree = quotient_degree_factor + 1
static int air_plan(p2hot_ctx *ctx, const char *what, const p2hot_air_program *pr, const uint64_t *public_inputs, size_t trace_width,
                    const uint64_t *alphas, unsigned nc, unsigned max_degree, AirPlan *pl) {
    if (!pr) P2_FAIL(ctx, P2HOT_EINVAL, "%s: null constraint program", what);
    if ((pr->num_insns && !pr->insns) || (pr->num_constants && !pr->constants))
        P2_FAIL(ctx, P2HOT_EINVAL, "%s: a program array is null but its count is not", what);
    if (pr->num_publics && !public_inputs) P2_FAIL(ctx, P2HOT_EINVAL, "%s: the program names %u public inputs and public_inputs is null", what, pr->num_publics);
    if (pr->num_temps > air::MAX_TEMPS)
        P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "%s: the program uses %u temp slots (p2hot_air_max_temps() = %u)", what, pr->num_temps, air::MAX_TEMPS);
    // the degree of every written temp slot in units of the trace's degree (saturating); ~0u: not written yet
    const u32 unwritten = ~0u, sat = 1u << 20;
    std::vector<u32> tdeg(pr->num_temps, unwritten);
    for (u32 k = 0; k < pr->num_insns; ++k) {
        const p2hot_air_insn &in = pr->insns[k];
        if (in.op > P2HOT_AIR_CONSTRAINT_LAST_ROW) P2_FAIL(ctx, P2HOT_EUNSUPPORTED, "%s: instruction %u: unknown op %u", what, k, in.op);
        const bool arith = in.op <= P2HOT_AIR_MUL;
        u32 deg[2] = {0, 0};
        for (int s = 0; s < (arith ? 2 : 1); ++s) {
            const u32 o = s ? in.b : in.a, kind = o >> air::KIND_SHIFT, idx = o & air::INDEX_MASK;
            const char side = s ? 'b' : 'a';
            switch (kind) {
                case P2HOT_AIR_LOCAL:
                case P2HOT_AIR_NEXT:
                    if (idx >= trace_width) P2_FAIL(ctx, P2HOT_EINVAL, "%s: instruction %u: operand %c reads column %u of a trace of %zu", what, k, side, idx, trace_width);
                    deg[s] = 1;
                    break;
                case P2HOT_AIR_PUBLIC:
                    if (idx >= pr->num_publics) P2_FAIL(ctx, P2HOT_EINVAL, "%s: instruction %u: operand %c reads public input %u of %u", what, k, side, idx, pr->num_publics);
                    break;
                case P2HOT_AIR_CONST:
                    if (idx >= pr->num_constants) P2_FAIL(ctx, P2HOT_EINVAL, "%s: instruction %u: operand %c reads constant %u of %u", what, k, side, idx, pr->num_constants);
                    break;
                case P2HOT_AIR_TEMP:
                    if (idx >= pr->num_temps) P2_FAIL(ctx, P2HOT_EINVAL, "%s: instruction %u: operand %c reads temp %u of %u", what, k, side, idx, pr->num_temps);
                    if (tdeg[idx] == unwritten) P2_FAIL(ctx, P2HOT_EINVAL, "%s: instruction %u: operand %c reads temp %u before any instruction wrote it", what, k, side, idx);
                    deg[s] = tdeg[idx];
                    break;
                default:
                    P2_FAIL(ctx, P2HOT_EINVAL, "%s: instruction %u: operand %c has the unknown kind %u", what, k, side, kind);
            }
        }
        if (arith) {
            if (in.dst >= pr->num_temps) P2_FAIL(ctx, P2HOT_EINVAL, "%s: instruction %u writes temp %u of %u", what, k, in.dst, pr->num_temps);
            tdeg[in.dst] = std::min(sat, in.op == P2HOT_AIR_MUL ? deg[0] + deg[1] : std::max(deg[0], deg[1]));
        } else {
            const u32 d = deg[0] + (in.op == P2HOT_AIR_CONSTRAINT_FIRST_ROW || in.op == P2HOT_AIR_CONSTRAINT_LAST_ROW ? 1 : 0);
            if (d > max_degree)
                P2_FAIL(ctx, P2HOT_EINVAL, "%s: instruction %u: a constraint of degree %u, above quotient_degree_factor + 1 = %u", what, k, d, max_degree);
        }
    }
    pl->insns.assign(pr->insns, pr->insns + pr->num_insns);
    pl->num_temps = pr->num_temps;
    pl->constants.resize(pr->num_constants);
    for (u32 k = 0; k < pr->num_constants; ++k) pl->constants[k] = gl::canon(pr->constants[k]);
    pl->publics.resize(pr->num_publics);
    for (u32 k = 0; k < pr->num_publics; ++k) pl->publics[k] = gl::canon(public_inputs[k]);
    pl->alphas.resize(nc);
    for (unsigned a = 0; a < nc; ++a) pl->alphas[a] = gl::canon(alphas[a]);
    return P2HOT_OK;
}

// the plan's arrays as one device block: alphas, constants, public inputs, then the instructions (16 bytes each)
static int air_blob_alloc(p2hot_ctx *ctx, AirPlan &pl, PoolBuf &d, air::Args *q) {
    const size_t na = pl.alphas.size(), ncst = pl.constants.size(), np = pl.publics.size();
    pl.blob.assign(na + ncst + np + 2 * pl.insns.size() + 1, 0);
    std::copy(pl.alphas.begin(), pl.alphas.end(), pl.blob.begin());
    std::copy(pl.constants.begin(), pl.constants.end(), pl.blob.begin() + na);
    std::copy(pl.publics.begin(), pl.publics.end(), pl.blob.begin() + na + ncst);
    if (!pl.insns.empty()) memcpy(pl.blob.data() + na + ncst + np, pl.insns.data(), pl.insns.size() * sizeof(p2hot_air_insn));
    P2_TRY(pool_alloc(ctx, pl.blob.size() * 8, &d.p));
    q->alphas = d.u(), q->constants = d.u() + na, q->publics = d.u() + na + ncst;
    q->insns = (const p2hot_air_insn *)(d.u() + na + ncst + np);
    q->num_insns = (unsigned)pl.insns.size();
    return P2HOT_OK;
}

// uploads the block and runs the interpreter over the 2^log_nq points; q holds everything but the program
static int air_enqueue(p2hot_ctx *ctx, AirPlan &pl, PoolBuf &d_blob, const air::Args &q, unsigned nc) {
    P2_HIP(ctx, hipMemcpyAsync(d_blob.p, pl.blob.data(), pl.blob.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    ProfScope prof(ctx, "stark_air_eval");
    const size_t shm = (size_t)(pl.num_temps ? pl.num_temps : 1) * air::BLOCK * 8;
    const dim3 grid(cdiv((size_t)1 << q.log_nq, air::BLOCK)), block(air::BLOCK);
    switch (nc) {
        case 1:
            P2_TRY(lds_opt_in(ctx, reinterpret_cast<const void *>(air::eval_kernel<1>), shm));
            P2HOT_LAUNCH((air::eval_kernel<1>), grid, block, shm, ctx->stream, q);
            break;
        case 2:
            P2_TRY(lds_opt_in(ctx, reinterpret_cast<const void *>(air::eval_kernel<2>), shm));
            P2HOT_LAUNCH((air::eval_kernel<2>), grid, block, shm, ctx->stream, q);
            break;
        case 3:
            P2_TRY(lds_opt_in(ctx, reinterpret_cast<const void *>(air::eval_kernel<3>), shm));
            P2HOT_LAUNCH((air::eval_kernel<3>), grid, block, shm, ctx->stream, q);
            break;
        default:
            P2_TRY(lds_opt_in(ctx, reinterpret_cast<const void *>(air::eval_kernel<4>), shm));
            P2HOT_LAUNCH((air::eval_kernel<4>), grid, block, shm, ctx->stream, q);
            break;
    }
    P2_LAUNCH_CHECK(ctx);
    return P2HOT_OK;
}
