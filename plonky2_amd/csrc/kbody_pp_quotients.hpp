// Kernel body fragment: #included inside pp_quotients_kernel and inside its M-proof form pp_quotients_many_kernel (plonk.hpp / gates.hpp /
// gates_recursion.hpp), which bind the same names to per-proof values.  One text for both, and the single-proof kernel's tokens --
// hence its code -- stay what they were.  No include guard on purpose.
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = (size_t)1 << a.log_n;
    if (i >= n) return;
    const u64 x = a.log_n ? ntt::root_pow(a.roots, (u32)(i << (32 - a.log_n))) : 1;
    const u64 bx = gl::mul(a.beta, x);
    u64 pn = 1, pd = 1;
    for (unsigned c = 0; c < a.num_chunks; ++c) {
        u64 d = 1;
        const unsigned j_end = (c + 1) * a.degree < a.num_routed ? (c + 1) * a.degree : a.num_routed;
        for (unsigned j = c * a.degree; j < j_end; ++j) {
            const u64 w = a.wires[(size_t)j * a.wires_stride + i];
            const u64 num = gl::add(gl::add(w, gl::mul(bx, a.k_is[j])), a.gamma);
            const u64 den = gl::add(gl::add(w, gl::mul(a.beta, a.sigmas[(size_t)j * a.sigmas_stride + i])), a.gamma);
            pn = gl::mul(pn, num);
            d = gl::mul(d, den);
        }
        pd = gl::mul(pd, d);
        a.dchunk[(size_t)c * n + i] = d;
        if (c + 1 < a.num_chunks) a.pp[(size_t)c * a.pp_stride + i] = pn;
    }
    if (gl::canon(pd) == 0) atomicOr(a.zero_flag, 1u);
    u64 inv = gl::inv(pd);  // PD_last^-1
    a.total[i] = gl::mul(pn, inv);
    for (unsigned c = a.num_chunks; c-- > 0;) {
        if (c + 1 < a.num_chunks) {
            u64 *q = a.pp + (size_t)c * a.pp_stride + i;
            *q = gl::mul(*q, inv);
        }
        inv = gl::mul(inv, a.dchunk[(size_t)c * n + i]);
    }
