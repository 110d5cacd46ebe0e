// lr_ckks_combine.hip -- out = a (+|-) b on the device for CKKS ciphertexts of any scale, level and degree: the element loops of
// evaluator.Add / AddNoMod / Sub / SubNoMod through evaluateInPlace (ckks/evaluator.go:227-342) -- MultByConst on the operand of the
// smaller scale (:712-730), the operation on the shared components (ring/ring.go:26, :48, :70, :94), CopyLvl of the surplus ones (:335,
// :339) and Sub's NegLvl on them (:186-192, :203-209) -- as ONE streaming pass (lr_stream.hpp): every operand row read once, the receiver
// row written once.  The same pass covers the steps between the products of the Chebyshev drivers: Add(C, C, C) before the Sub
// (double_a; computePowerBasisCheby, ckks/chebyshev_evaluation.go:92), AddConst on component 0 (:433, :441) and a MultByConst whose
// words differ between the halves.  The element operations are lr_ewise's and lr_half_scalar_op's, in their order, on values that need
// not be canonical.
#include "lattigo_ring.h"
#include "lr_stream.hpp"

namespace lr {

// The limb on blockIdx.y, batch member and component on blockIdx.z = batch * u + b.  Every flag, the operation and both degrees are the
// launch's and u is the workgroup's: each branch below is wave-uniform, and the limb's constants are read from the kernel arguments at
// wave-uniform addresses (scalar loads).  An element is read before it is written by the same lane, so out_u may be a_u or b_u.
__global__ __launch_bounds__(256) void ckks_combine_kernel(CombineLaunch L) {
    const int limb = blockIdx.y;
    const int comps = combine_comps(L.deg_a, L.deg_b);
    const int batch = gridDim.z / comps;
    const long long b = blockIdx.z % batch;
    const int u = blockIdx.z / batch;
    const u64 q = L.lp[limb].q, qinv = L.lp[limb].qinv;
    const u64 *kw = L.k + limb * kCombineLimbWords;                    // ma_lo, ma_hi, mb_lo, mb_hi, add_lo, add_hi
    const bool has_x = u <= L.deg_a, has_y = u <= L.deg_b;
    const bool add = L.has_add && u == 0;                              // AddConst touches value[0] only
    const bool subtract = L.op == LR_SUB || L.op == LR_SUB_NOMOD;
    const long long row = (long long)limb * L.n;
    const ulonglong2 *pa = has_x ? row_in(L.a[u], b, L.a_stride[u], row) : nullptr;
    const ulonglong2 *pb = has_y ? row_in(L.b[u], b, L.b_stride[u], row) : nullptr;
    ulonglong2 *po = row_out(L.out[u], b, L.out_stride[u], row);
    const int pairs = L.n >> 1, half = L.n >> 2;       // n / 2 coefficients = n / 4 pairs per half
    LR_FOR_PAIRS(e, pairs) {
        const bool low = e < half;
        ulonglong2 x = make_ulonglong2(0, 0), y = x, r;
        if (has_x) x = ld_shared(pa, L.a_stride[u], e);
        if (has_y) y = ld_shared(pb, L.b_stride[u], e);
        if (has_x) {
            if (L.double_a) x = add2(x, x, q);                                                   // Add(C, C, C), ring/ring.go:26
            if (L.mult_a) {
                const u64 slo = kw[0], shi = kw[1];                                              // (both read: the addresses stay wave-uniform)
                x = muls2(x, low ? slo : shi, q, qinv);                                          // MultByConst :715, :728
            }
        }
        if (has_y && L.mult_b) {
            const u64 slo = kw[2], shi = kw[3];
            y = muls2(y, low ? slo : shi, q, qinv);
        }
        if (has_x && has_y) {
            switch (L.op) {
            case LR_ADD: r = add2(x, y, q); break;                                               // ring/ring.go:26
            case LR_ADD_NOMOD: r = add2_nomod(x, y); break;                                      // :48
            case LR_SUB: r = sub2(x, y, q); break;                                               // :70
            default: r = sub2_nomod(x, y, q); break;                                             // :94
            }
        } else if (has_x) {
            r = x;                                                                               // CopyLvl :335
        } else {
            r = subtract ? neg2(y, q) : y;                                                       // CopyLvl :339, NegLvl :190 / :207
        }
        if (add) {
            const u64 slo = kw[4], shi = kw[5];
            const u64 s = low ? slo : shi;
            r = add2(r, make_ulonglong2(s, s), q);                                               // AddConst :433, :441
        }
        st_stream(po + e, r);
    }
}

hipError_t launch_ckks_combine(const CombineLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    return launch_kernel(ckks_combine_kernel, pair_grid(L.n, (unsigned)limbs, (unsigned)(combine_comps(L.deg_a, L.deg_b) * batch)), dim3(256), 0, stream, L);
}

}  // namespace lr
