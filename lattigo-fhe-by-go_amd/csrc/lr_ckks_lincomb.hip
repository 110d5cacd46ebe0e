// lr_ckks_lincomb.hip -- res = c0 + sum_k c_k ct_k on the device: the element loops of evaluatePolyFromPowerBasis' chain (ckks/
// polynomial_evaluation.go:142-159), AddConst (ckks/evaluator.go:429-445) once and per term MultByConst on the receiver where the
// reference equalises scales (:712-730) and MultByConstAndAdd (:588-606), as ONE streaming pass (lr_stream.hpp): every term row read
// once, the receiver row written once -- T + 1 row passes where the call-by-call route (lr_half_scalar_op per term and component) moves
// 3 T to 5 T.  The element operations are lr_half_scalar_op's, in its order, on values that need not be canonical.
#include "lr_stream.hpp"

namespace lr {

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

}  // namespace lr
