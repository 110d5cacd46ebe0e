// lr_ckks_chain.hip -- the pass in front of the key switch in every step of an accumulating CKKS rotation chain (lr_ckks_rotate_chain,
// lr_ckks_chain.cpp; the slot-sum loop RotateColumns; Add): both PermuteNTT calls of evaluator.permuteNTT (ckks/evaluator.go:1458-1459)
// and the first component's addition as ONE launch.
#include "lattigo_ring.h"
#include "lr_stream.hpp"

namespace lr {

// Grid: row blocks on x, the limb on y, 2 * member + component on z; one coefficient per lane.  With pi = galois_index of g:
//   component 0:  plus0[j] = CRed(a0[pi(j)] + a0[j])
//   component 1:  cx[j]    = a1[pi(j)]
// The key switch that follows adds plus0 to its first result in its last pass: out0 = CRed(p0 + plus0).  The reference's slot-sum step
// is out0 = CRed(CRed(e0 + p0) + a0) with e0 = a0[pi(j)] (permuteNTT :1466, then Add); for a0 and p0 in [0, q) every CRed there is a
// full reduction of a sum below 2q, so both associations give (e0 + p0 + a0) mod q: the same bits.  That is the domain the header states.
//
// Access pattern.  In the bit-reversed order of the NTT domain pi(j) = brev(t) with r = brev(j) and
//   t = (g (2 r + 1) - 1) / 2 mod N = g r + (g - 1) / 2 mod N           (ring.PermuteNTTIndex, ring/ring_galois.go:29-52).
// A wave holds 64 consecutive positions j = 64 w + l, l = 0 .. 63, so r = brev6(l) * N/64 + brev(w) and
//   t = [g brev(w) + (g - 1) / 2] + g brev6(l) * N/64 mod N.
// The bracket is the wave's; the other term touches only the top six bits of t.  So the low log2(N) - 6 bits of t -- the HIGH bits of
// pi(j) -- are the same for the whole wave: it gathers from one aligned block of 64 words (512 bytes, four lines), and since g is odd
// l -> (c + g brev6(l)) mod 64 is a bijection: it reads each word of that block once.  The gather moves whole lines, like a copy; no LDS
// staging and no limit on the degree (the BFV pass permutes in the coefficient domain, where the stride is g words, and needs the row
// in LDS).  The load of a0[j] and both stores are contiguous.  Plain loads and stores: the inverse transform and the epilogue of
// the key switch read cx and plus0 next.
__global__ __launch_bounds__(256) void ckks_chain_step_kernel(CkksChainStepLaunch L) {
    const int limb = blockIdx.y, k = blockIdx.z & 1;
    const long long b = blockIdx.z >> 1, row = (long long)limb * L.n;
    const u64 *pin = (k ? L.a1 + b * L.a1_stride : L.a0 + b * L.a0_stride) + row;
    u64 *pout = (k ? L.cx + b * L.cx_stride : L.plus0 + b * L.plus_stride) + row;
    const u64 q = L.lp[limb].q;
    const u32 mask2 = 2u * (u32)L.n - 1u;
    const int logn = L.logn;
    LR_FOR_PAIRS(j, L.n) {
        u64 x = pin[galois_index((u32)j, L.gen, mask2, logn)];       // :1458 / :1459
        if (k == 0) x = cred(x + pin[j], q);                         // Add, first component (k is the workgroup's: wave-uniform)
        pout[j] = x;
    }
}

hipError_t launch_ckks_chain_step(const CkksChainStepLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    return launch_kernel(ckks_chain_step_kernel, coeff_grid(L.n, (unsigned)limbs, 2u * (unsigned)batch), dim3(256), 0, stream, L);
}

}  // namespace lr
