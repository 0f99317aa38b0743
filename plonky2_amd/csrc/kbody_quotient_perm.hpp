// Kernel body fragment: #included inside quotient_perm_kernel and inside its M-proof form quotient_perm_many_kernel (plonk.hpp / gates.hpp /
// gates_recursion.hpp), which bind the same names to per-proof values.  One text for both, and the single-proof kernel's tokens --
// hence its code -- stay what they were.  No include guard on purpose.
    const size_t L = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nq = (size_t)1 << q.log_nq;
    if (L >= nq) return;
    const size_t i = q.log_nq ? (size_t)(__brevll((unsigned long long)L) >> (64 - q.log_nq)) : 0;
    const size_t i_next = (i + ((size_t)1 << q.qbits)) & (nq - 1);
    const size_t L_next = q.log_nq ? (size_t)(__brevll((unsigned long long)i_next) >> (64 - q.log_nq)) : 0;
    const u64 x = gl::mul(gl::COSET_SHIFT, q.log_nq ? ntt::root_pow(q.roots, (u32)(i << (32 - q.log_nq))) : (u64)1);
    const size_t r = i & (((size_t)1 << q.qbits) - 1);
    // L_0(x) = Z_H(x) / (n (x - 1))  (zero_poly_coset.rs:58-61)
    const u64 l0 = gl::mul(q.zh[r], q.inv_nx1[L]);
    const unsigned num_prods = q.num_chunks - 1;
    const unsigned degree = DEG ? (unsigned)DEG : q.degree;
    u64 zx[NC], acc[NC][NC], pw[NC], res[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        zx[c] = q.zs[(size_t)c * q.zs_stride + L];
#pragma unroll
        for (int a = 0; a < NC; ++a) acc[a][c] = 0;
        pw[c] = 1;  // alpha_c^chunk
    }
    // terms 0 .. NC-1: L_0(x) (Z_c(x) - 1)
#pragma unroll
    for (int a = 0; a < NC; ++a) {
        u64 s = 0, p = 1;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            s = gl::mul_add(gl::mul(l0, gl::sub(zx[c], 1)), p, s);
            p = gl::mul(p, q.alphas[a]);
        }
        res[a] = s;
    }
    u64 prev[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) prev[c] = zx[c];
    constexpr int BUF = DEG ? DEG : 1;
    u64 wb[BUF], sb[BUF];  // the chunk in flight (DEG > 0)
    if (DEG) {
#pragma unroll
        for (int t = 0; t < BUF; ++t) {
            const unsigned j = (unsigned)t < q.num_routed ? (unsigned)t : q.num_routed - 1;
            wb[t] = q.wires[(size_t)j * q.wires_stride + L];
            sb[t] = q.sigmas[(size_t)j * q.sigmas_stride + L];
        }
    }
    for (unsigned ch = 0; ch < q.num_chunks; ++ch) {
        u64 pn[NC], pd[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) pn[c] = pd[c] = 1;
        const unsigned j0 = ch * degree, j_end = j0 + degree < q.num_routed ? j0 + degree : q.num_routed;
        // the "next" value of this chunk's check (a partial product of x, or Z(g x) for the last chunk): loaded early too
        u64 nextv[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c)
            nextv[c] = ch == num_prods ? q.zs[(size_t)c * q.zs_stride + L_next] : q.zs[((size_t)NC + (size_t)c * num_prods + ch) * q.zs_stride + L];
        if (DEG) {
            u64 wc[BUF], sc[BUF];
#pragma unroll
            for (int t = 0; t < BUF; ++t) wc[t] = wb[t], sc[t] = sb[t];
            if (ch + 1 < q.num_chunks) {  // the next chunk's loads go out before this chunk's arithmetic
#pragma unroll
                for (int t = 0; t < BUF; ++t) {
                    const unsigned jn = j0 + degree + (unsigned)t, j = jn < q.num_routed ? jn : q.num_routed - 1;
                    wb[t] = q.wires[(size_t)j * q.wires_stride + L];
                    sb[t] = q.sigmas[(size_t)j * q.sigmas_stride + L];
                }
            }
            if constexpr (NC == 2) {
                // eight multiplications per routed wire as hand-scheduled streams (gl_mul3.hpp: 14 instructions each, where the
                // compiler's 64-bit code spends ~34 per multiply-reduce here): {bk0 x + wg0, bk1 x + wg1, beta0 sigma + wg0}, then
                // {beta1 sigma + wg1, pn0 n0, pn1 n1}, then {pd0 d0, pd1 d1}
#pragma unroll
                for (int t = 0; t < BUF; ++t) {
                    if (j0 + (unsigned)t < j_end) {
                        const u64 wg0 = gl::add_canon(wc[t], q.gammas[0]), wg1 = gl::add_canon(wc[t], q.gammas[1]);
                        // (the additions ride the streams' multiply-adds: gl::mad3)
                        const u64 a1[3] = {q.bk[j0 + t], q.bk[(size_t)q.num_routed + j0 + t], q.betas[0]}, b1[3] = {x, x, sc[t]}, c1[3] = {wg0, wg1, wg0};
                        u64 r1[3];
                        gl::mad3(a1, b1, c1, r1);  // n0, n1, d0
                        const u64 a2[3] = {q.betas[1], pn[0], pn[1]}, b2[3] = {sc[t], r1[0], r1[1]}, c2[3] = {wg1, 0, 0};
                        u64 r2[3];
                        gl::mad3(a2, b2, c2, r2);  // d1, pn0 n0, pn1 n1
                        pn[0] = r2[1], pn[1] = r2[2];
                        const u64 d0 = r1[2], d1 = r2[0];
                        const u64 a3[2] = {pd[0], pd[1]}, b3[2] = {d0, d1};
                        u64 r3[2];
                        gl::mul2(a3, b3, r3);
                        pd[0] = r3[0], pd[1] = r3[1];
                    }
                }
            } else {
#pragma unroll
                for (int t = 0; t < BUF; ++t) {
                    if (j0 + (unsigned)t < j_end) {
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            const u64 wg = gl::add(wc[t], q.gammas[c]);
                            pn[c] = gl::mul(pn[c], gl::mul_add(q.bk[(size_t)c * q.num_routed + j0 + t], x, wg));
                            pd[c] = gl::mul(pd[c], gl::mul_add(q.betas[c], sc[t], wg));
                        }
                    }
                }
            }
        } else {
            for (unsigned j = j0; j < j_end; ++j) {
                const u64 w = q.wires[(size_t)j * q.wires_stride + L], sg = q.sigmas[(size_t)j * q.sigmas_stride + L];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const u64 wg = gl::add(w, q.gammas[c]);
                    pn[c] = gl::mul(pn[c], gl::mul_add(q.bk[(size_t)c * q.num_routed + j], x, wg));
                    pd[c] = gl::mul(pd[c], gl::mul_add(q.betas[c], sg, wg));
                }
            }
        }
        if constexpr (NC == 2 && DEG != 0) {  // the chunk's check and its place in the alpha sums, as streams too
            const u64 a1[3] = {prev[0], prev[1], nextv[0]}, b1[3] = {pn[0], pn[1], pd[0]};
            u64 r1[3];
            gl::mul3(a1, b1, r1);
            const u64 a2[3] = {nextv[1], pw[0], pw[1]}, b2[3] = {pd[1], q.alphas[0], q.alphas[1]}, z3[3] = {0, 0, 0};
            u64 r2[3];
            gl::mad3(a2, b2, z3, r2);
            const u64 term0 = gl::sub(r1[0], r1[2]), term1 = gl::sub(r1[1], r2[0]);
            const u64 a3[3] = {term0, term0, term1}, b3[3] = {pw[0], pw[1], pw[0]}, c3[3] = {acc[0][0], acc[1][0], acc[0][1]};
            u64 r3[3];
            gl::mad3(a3, b3, c3, r3);
            acc[0][0] = r3[0], acc[1][0] = r3[1], acc[0][1] = r3[2];
            acc[1][1] = gl::mul_add(term1, pw[1], acc[1][1]);
            pw[0] = r2[1], pw[1] = r2[2];
            prev[0] = nextv[0], prev[1] = nextv[1];
        } else {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const u64 term = gl::sub(gl::mul(prev[c], pn[c]), gl::mul(nextv[c], pd[c]));
                prev[c] = nextv[c];
#pragma unroll
                for (int a = 0; a < NC; ++a) acc[a][c] = gl::mul_add(term, pw[a], acc[a][c]);
            }
#pragma unroll
            for (int a = 0; a < NC; ++a) pw[a] = gl::mul(pw[a], q.alphas[a]);
        }
    }
    const u64 zinv = q.zh[((size_t)1 << q.qbits) + r];
#pragma unroll
    for (int a = 0; a < NC; ++a) {
        u64 s = res[a];
#pragma unroll
        for (int c = 0; c < NC; ++c) s = gl::mul_add(acc[a][c], q.base[a][c], s);
        if (q.gate_sums) s = gl::mul_add(q.alpha_k[a], q.gate_sums[(size_t)a * nq + i], s);
        q.out[(size_t)a * nq + i] = gl::canon(gl::mul(s, zinv));
    }
