// lr_ckks_eval.hip -- the streaming passes of the CKKS evaluator unit (lr_abi_ckks_eval.cpp): the linear combination, Add / Sub of any
// scale, level and degree, the step pass of an accumulating rotation chain and the tail pass of a power basis.
#include "lattigo_ring.h"
#include "lr_stream.hpp"

namespace lr {

// lr_ckks_lincomb -- res = c0 + sum_k c_k ct_k on the device: the element loops of evaluatePolyFromPowerBasis' chain (ckks/
// polynomial_evaluation.go:142-159), AddConst (ckks/evaluator.go:429-445) once and per term MultByConst on the receiver where the
// reference equalises scales (:712-730) and MultByConstAndAdd (:588-606), as ONE streaming pass (lr_stream.hpp): every term row read
// once, the receiver row written once -- T + 1 row passes where the call-by-call route (lr_half_scalar_op per term and component) moves
// 3 T to 5 T.  The element operations are lr_half_scalar_op's, in its order, on values that need not be canonical.

// The limb on blockIdx.y (relative to LinCombLaunch::limb0), batch member and component on blockIdx.z = 2 b + u.  The accumulator of a
// coefficient pair stays in registers over the terms; the terms' loads do not depend on it, so kLoadsAhead of them are issued before the
// first multiply.  The term count and the pre-multiplier mask are the launch's: every branch on them is wave-uniform, and the limb's
// constants are read from the kernel arguments at wave-uniform addresses (scalar loads).
constexpr int kLoadsAhead = 4;
static_assert(kLoadsAhead == 4, "the kernel's tail switch names the group sizes below kLoadsAhead");

// G terms from k0 on as straight-line code: their loads, then the arithmetic in the terms' order as the loads arrive
template <int G, class Load, class Step>
LR_D void term_group(int k0, const Load &load, const Step &step) {
    ulonglong2 x[G];
#pragma unroll
    for (int j = 0; j < G; ++j) x[j] = load(k0 + j);
#pragma unroll
    for (int j = 0; j < G; ++j) step(k0 + j, x[j]);
}

__global__ __launch_bounds__(256) void ckks_lincomb_kernel(LinCombLaunch L) {
    const int y = blockIdx.y, limb = L.limb0 + y;
    const long long b = blockIdx.z >> 1;
    const int u = blockIdx.z & 1;
    const u64 q = L.lp[limb].q, qinv = L.lp[limb].qinv;
    const int count = L.count;
    const u64 *kw = L.k + y * lincomb_limb_words(count, L.has_add);     // this limb's constants
    const u64 *tw = kw + (L.has_add ? 2 : 0);                           // (pre, lo, hi) per term
    const bool add = L.has_add && u == 0;                               // AddConst touches value[0] only
    const long long row = (long long)limb * L.n;
    ulonglong2 *po = row_out(L.out[u], b, L.out_stride[u], row);
    const int pairs = L.n >> 1, half = L.n >> 2;       // n / 2 coefficients = n / 4 pairs per half
    LR_FOR_PAIRS(e, pairs) {
        const bool low = e < half;
        ulonglong2 acc = L.accumulate ? ld_stream(po + e) : make_ulonglong2(0, 0);
        if (add) {
            const u64 slo = kw[0], shi = kw[1];
            const u64 s = low ? slo : shi;
            acc = add2(acc, make_ulonglong2(s, s), q);                                           // :433, :441
        }
        const auto load = [&](int k) { return ld_stream(row_in(L.term[k].c[u], b, L.term[k].stride[u], row) + e); };
        const auto step = [&](int k, ulonglong2 x) {
            const u64 *t = tw + 3 * k;
            const u64 slo = t[1], shi = t[2];                                                    // (both read: the addresses stay wave-uniform)
            if ((L.pre_mask >> k) & 1u) acc = muls2(acc, t[0], q, qinv);                           // MultByConst on the receiver, :715, :728
            const u64 s = low ? slo : shi;
            acc = muladd2(acc, x, make_ulonglong2(s, s), q, qinv);                                 // :591, :604
        };
        int k0 = 0;
        for (; k0 + kLoadsAhead <= count; k0 += kLoadsAhead) term_group<kLoadsAhead>(k0, load, step);
        switch (count - k0) {                                      // the last count % kLoadsAhead terms, as one shorter group
        case 3: term_group<3>(k0, load, step); break;
        case 2: term_group<2>(k0, load, step); break;
        case 1: term_group<1>(k0, load, step); break;
        default: break;
        }
        st_stream(po + e, acc);
    }
}

hipError_t launch_ckks_lincomb(const LinCombLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    return launch_kernel(ckks_lincomb_kernel, pair_grid(L.n, (unsigned)limbs, 2u * (unsigned)batch), dim3(256), 0, stream, L);
}

// lr_ckks_combine -- out = a (+|-) b on the device for CKKS ciphertexts of any scale, level and degree: the element loops of
// evaluator.Add / AddNoMod / Sub / SubNoMod through evaluateInPlace (ckks/evaluator.go:227-342) -- MultByConst on the operand of the
// smaller scale (:712-730), the operation on the shared components (ring/ring.go:26, :48, :70, :94), CopyLvl of the surplus ones (:335,
// :339) and Sub's NegLvl on them (:186-192, :203-209) -- as ONE streaming pass (lr_stream.hpp): every operand row read once, the receiver
// row written once.  The same pass covers the steps between the products of the Chebyshev drivers: Add(C, C, C) before the Sub
// (double_a; computePowerBasisCheby, ckks/chebyshev_evaluation.go:92), AddConst on component 0 (:433, :441) and a MultByConst whose
// words differ between the halves.  The element operations are lr_ewise's and lr_half_scalar_op's, in their order, on values that need
// not be canonical.

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

// lr_ckks_rotate_chain -- the pass in front of the key switch in every step of an accumulating CKKS rotation chain (the slot-sum loop RotateColumns; Add): both PermuteNTT calls of evaluator.permuteNTT (ckks/evaluator.go:1458-1459)
// and the first component's addition as ONE launch.

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

// lr_ckks_power_basis -- what follows MulRelin and Rescale in every product of a CKKS power basis (computePowerBasis, ckks/polynomial_evaluation.go:76-93, and computePowerBasisCheby, ckks/chebyshev_evaluation.go:
// 60-101), for all products of one chunk as ONE streaming pass (lr_stream.hpp): the staging pair read once, C[n] written once where the
// caller wants it.  It stands for the scatter of the merged products to their polys and, per product, the lr_ckks_combine call of the
// Chebyshev step.

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
