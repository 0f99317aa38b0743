// Kernel body fragment: #included inside pp_carries_kernel and inside its M-proof form pp_carries_many_kernel (plonk.hpp / gates.hpp /
// gates_recursion.hpp), which bind the same names to per-proof values.  One text for both, and the single-proof kernel's tokens --
// hence its code -- stay what they were.  No include guard on purpose.
    __shared__ u64 s[1024];
    const unsigned tid = threadIdx.x;
    const size_t lo = (size_t)tid * per, hi = lo + per < n_chunks ? lo + per : n_chunks;
    u64 loc = 1;
    for (size_t m = lo; m < hi; ++m) loc = gl::mul(loc, prod[m]);
    s[tid] = loc;
    __syncthreads();
    for (unsigned d = 1; d < 1024; d <<= 1) {  // inclusive Hillis-Steele scan
        u64 f = 1;
        if (tid >= d) f = s[tid - d];
        __syncthreads();
        s[tid] = gl::mul(s[tid], f);
        __syncthreads();
    }
    u64 c = tid ? s[tid - 1] : 1;
    for (size_t m = lo; m < hi; ++m) {
        carry[m] = c;
        c = gl::mul(c, prod[m]);
    }
