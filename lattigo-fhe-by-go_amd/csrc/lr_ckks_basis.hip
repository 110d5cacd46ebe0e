// lr_ckks_basis.hip -- what follows MulRelin and Rescale in every product of a CKKS power basis (lr_ckks_power_basis,
// lr_ckks_basis.cpp; computePowerBasis, ckks/polynomial_evaluation.go:76-93, and computePowerBasisCheby, ckks/chebyshev_evaluation.go:
// 60-101), for all products of one chunk as ONE streaming pass (lr_stream.hpp): the staging pair read once, C[n] written once where the
// caller wants it.  It stands for the scatter of the merged products to their polys and, per product, the lr_ckks_combine call of the
// Chebyshev step.
#include "lattigo_ring.h"
#include "lr_stream.hpp"

namespace lr {

// The limb on blockIdx.y; component and member on blockIdx.z = u * members + m with m = k * batch + b: product k of the chunk, batch
// member b.  The staging pair holds its 2 * members polys back to back in that very order.  Per element, with q the limb's modulus:
//   x = staging_u[m]                                                    the rescaled product
//   tail 0:  r = x                                                      computePowerBasis: nothing follows the Rescale
//   tail 1:  x = CRed(x + x)                                            Add(C[n], C[n], C[n]), chebyshev_evaluation.go:92
//            mult_side 1: x = MRed(x, mult[k])   2: y = MRed(y, mult[k])     MultByConst on the operand of the smaller scale,
//            r = CRed((x + q) - y)   with y = C[1]_u[b]                      Sub(C[n], C[c], C[n]) :98 through evaluateInPlace
//   tail 2:  x = CRed(x + x);  r = u == 0 ? CRed(x + add[k]) : x        Add :92, AddConst(C[n], -1, C[n]) :96 (value[0] only; the
//                                                                       constant is real: one word for both halves of the row)
// -- lr_ckks_combine's element operations in its order (ckks_combine_kernel with double_a, mult_a / mult_b, LR_SUB, has_add).
// k, u and the limb are the workgroup's: the product's entry, its two words and the limb's constants are read at wave-uniform addresses
// (scalar loads) and every branch is wave-uniform.  The staged element is read once and streams past the caches; C[1] is read by every
// product of the chunk and goes through them.
__global__ __launch_bounds__(256) void basis_tail_kernel(BasisTailLaunch L) {
    const int limb = blockIdx.y;
    const int members = gridDim.z >> 1;
    const int u = (int)blockIdx.z >= members ? 1 : 0;
    const int m = (int)blockIdx.z - u * members;
    const int k = m / L.batch;
    const long long b = m - k * L.batch;
    const BasisTailProduct P = L.products[k];
    const u64 q = L.lp[limb].q, qinv = L.lp[limb].qinv;
    const u64 mult = L.mult[(long long)k * L.row + limb], addw = L.add[(long long)k * L.row + limb];
    const long long row = (long long)limb * L.n;
    const ulonglong2 *px = row_in(L.stage, blockIdx.z, L.stage_stride, row);
    const ulonglong2 *py = row_in(L.c1[u], b, L.c1_stride[u], row);
    ulonglong2 *po = row_out(P.out[u], b, P.out_stride, row);
    const int pairs = L.n >> 1;
    LR_FOR_PAIRS(e, pairs) {
        ulonglong2 x = ld_stream(px + e), r;
        if (P.tail == 0) {
            r = x;
        } else {
            x = add2(x, x, q);                                                                   // Add(C, C, C), ring/ring.go:26
            if (P.tail == 1) {
                ulonglong2 y = py[e];
                if (P.mult_side == 1) x = muls2(x, mult, q, qinv);                               // MultByConst :715, :728
                if (P.mult_side == 2) y = muls2(y, mult, q, qinv);
                r = sub2(x, y, q);                                                               // ring/ring.go:70
            } else {
                r = u == 0 ? add2(x, make_ulonglong2(addw, addw), q) : x;                        // AddConst :433, :441
            }
        }
        st_stream(po + e, r);
    }
}

hipError_t launch_ckks_basis_tail(const BasisTailLaunch &L, int limbs, int products, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, products)) return verdict_error(v);
    return launch_kernel(basis_tail_kernel, pair_grid(L.n, (unsigned)limbs, 2u * (unsigned)(products * L.batch)), dim3(256), 0, stream, L);
}

}  // namespace lr
