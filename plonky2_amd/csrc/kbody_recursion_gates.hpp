// Kernel body fragment: #included inside recursion_gates_kernel and inside its M-proof form recursion_gates_many_kernel (plonk.hpp / gates.hpp /
// gates_recursion.hpp), which bind the same names to per-proof values.  One text for both, and the single-proof kernel's tokens --
// hence its code -- stay what they were.  No include guard on purpose.
    const size_t L = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nq = (size_t)1 << q.log_nq;
    if (L >= nq) return;
    const size_t i = q.log_nq ? (size_t)(__brevll((unsigned long long)L) >> (64 - q.log_nq)) : 0;
    const u64 *w = q.wires + L, *lc = q.consts + (size_t)q.consts_first * q.consts_stride + L;
    auto wire = [&](unsigned c) { return w[(size_t)c * q.wires_stride]; };
    auto wext = [&](unsigned c) { return gl::ext2{w[(size_t)c * q.wires_stride], w[(size_t)(c + 1) * q.wires_stride]}; };
    u64 res[NC];
#pragma unroll
    for (int a = 0; a < NC; ++a) res[a] = 0;
    for (unsigned gi = 0; gi < q.num_gates; ++gi) {
        const p2hot_gate &g = q.gates[gi];
        u64 acc[NC];
#pragma unroll
        for (int a = 0; a < NC; ++a) acc[a] = 0;
        auto put = [&](unsigned j, u64 term) {  // constraint j of this gate
#pragma unroll
            for (int a = 0; a < NC; ++a) acc[a] = gl::mul_add(term, q.apow[(size_t)a * q.apow_stride + j], acc[a]);
        };
        auto put2 = [&](unsigned j, gl::ext2 x, gl::ext2 y) {  // the two components of x - y
            put(j, gl::sub(x.a0, y.a0));
            put(j + 1, gl::sub(x.a1, y.a1));
        };
        switch (g.kind) {
            case P2HOT_GATE_REDUCING:        // reducing.rs:107-127
            case P2HOT_GATE_REDUCING_EXT: {  // reducing_extension.rs:109-128
                const bool ext = g.kind == P2HOT_GATE_REDUCING_EXT;
                const unsigned n = g.param0, accs = 6 + (ext ? 2 * n : n);
                const gl::ext2 alpha = wext(2);
                gl::ext2 cur = wext(4);
                for (unsigned k = 0; k < n; ++k) {
                    gl::ext2 t = gl::ext_mul(cur, alpha);
                    if (ext) {
                        t = gl::ext_add(t, wext(6 + 2 * k));
                    } else {
                        t.a0 = gl::add(t.a0, wire(6 + k));
                    }
                    cur = wext(k == n - 1 ? 0 : accs + 2 * k);  // the last accumulator is the output; acc continues from the WIRE
                    put2(2 * k, t, cur);
                }
                break;
            }
            case P2HOT_GATE_EXPONENTIATION: {  // exponentiation.rs:210-243: power bits little endian on the wires, walked big endian
                const unsigned n = g.param0;
                const u64 base = wire(0);
                u64 prev = 1;
                for (unsigned k = 0; k < n; ++k) {
                    const u64 bit = wire(n - k), inter = wire(2 + n + k);
                    put(k, gl::sub(gl::mul(prev, gl::add(gl::mul(bit, base), gl::sub(1, bit))), inter));
                    prev = gl::sqr(inter);
                }
                put(n, gl::sub(wire(1 + n), wire(1 + 2 * n)));
                break;
            }
            case P2HOT_GATE_RANDOM_ACCESS: {  // random_access.rs:302-343
                const unsigned bits = ra_bits(g), extra = ra_extra(g), copies = g.param0, vec = 1u << bits, per = 2 + vec;
                unsigned j = 0;
                for (unsigned c = 0; c < copies; ++c) {
                    const unsigned first = per * c, bit0 = per * copies + extra + c * bits;
                    u64 b[MAX_ACCESS_BITS];
#pragma unroll
                    for (unsigned l = 0; l < MAX_ACCESS_BITS; ++l) {
                        b[l] = l < bits ? wire(bit0 + l) : 0;
                        if (l < bits) put(j++, gl::mul(b[l], gl::sub(b[l], 1)));
                    }
                    u64 index = 0;
#pragma unroll
                    for (int l = MAX_ACCESS_BITS - 1; l >= 0; --l)
                        if ((unsigned)l < bits) index = gl::add(gl::add(index, index), b[l]);
                    put(j++, gl::sub(index, wire(first)));
                    // the pairwise fold x + b_l (y - x), level l by bit l, as a binary counter over the items in wire order: item t
                    // enters at level 0 and every trailing one-bit of t combines it with the waiting left half of that level
                    u64 stack[MAX_ACCESS_BITS], cur = 0;
#pragma unroll
                    for (unsigned l = 0; l < MAX_ACCESS_BITS; ++l) stack[l] = 0;
                    for (unsigned t = 0; t < vec; ++t) {
                        cur = wire(first + 2 + t);
                        bool carry = true;  // wave-uniform: t is
#pragma unroll
                        for (unsigned l = 0; l < MAX_ACCESS_BITS; ++l) {
                            if (carry && (t >> l & 1u)) {
                                cur = gl::mul_add(b[l], gl::sub(cur, stack[l]), stack[l]);
                            } else if (carry) {
                                stack[l] = cur;
                                carry = false;
                            }
                        }
                    }
                    put(j++, gl::sub(cur, wire(first + 1)));
                }
                for (unsigned k = 0; k < extra; ++k) put(j++, gl::sub(lc[(size_t)k * q.consts_stride], wire(per * copies + k)));
                break;
            }
            case P2HOT_GATE_COSET_INTERPOLATION: {  // coset_interpolation.rs:251-298, partial_interpolate :553-580
                const unsigned sb = g.param0, d = g.param1, n = 1u << sb, ni = (n - 2) / (d - 1), inter = 1 + 2 * n + 4;
                const u64 ninv = q.ninv[sb];
                const gl::ext2 shifted = wext(inter + 4 * ni);
                {
                    const u64 shift = wire(0);
                    put2(0, wext(1 + 2 * n), gl::ext2{gl::mul(shifted.a0, shift), gl::mul(shifted.a1, shift)});
                }
                gl::ext2 eval{0, 0}, prod{1, 0};
                auto walk = [&](unsigned from, unsigned to) {
                    for (unsigned k = from; k < to; ++k) {
                        const u64 xk = q.dom[k << (MAX_SUBGROUP_BITS - sb)], wk = gl::mul(xk, ninv);
                        const gl::ext2 v = wext(1 + 2 * k), term{gl::sub(shifted.a0, xk), shifted.a1};
                        eval = gl::ext_add(gl::ext_mul(eval, term), gl::ext_mul(gl::ext2{gl::mul(v.a0, wk), gl::mul(v.a1, wk)}, prod));
                        prod = gl::ext_mul(prod, term);
                    }
                };
                walk(0, d);
                for (unsigned k = 0; k < ni; ++k) {
                    const gl::ext2 ie = wext(inter + 2 * k), ip = wext(inter + 2 * ni + 2 * k);
                    put2(2 + 4 * k, ie, eval);
                    put2(4 + 4 * k, ip, prod);
                    eval = ie, prod = ip;  // the walk continues from the WIRES
                    const unsigned from = 1 + (d - 1) * (k + 1), to = from + d - 1 < n ? from + d - 1 : n;
                    walk(from, to);
                }
                put2(2 + 4 * ni, wext(1 + 2 * n + 2), eval);
                break;
            }
            default: break;
        }
        const u64 f = filter(g, q.consts[(size_t)g.selector_index * q.consts_stride + L], q.num_selectors > 1);
#pragma unroll
        for (int a = 0; a < NC; ++a) res[a] = gl::mul_add(f, acc[a], res[a]);
    }
#pragma unroll
    for (int a = 0; a < NC; ++a) {
        u64 *o = q.out + (size_t)a * nq + i;
        *o = gl::canon(gl::add(*o, res[a]));
    }
