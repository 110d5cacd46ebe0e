// lr_collective.hip -- the kernels of collective key switching (lr_collective.cpp): what CKSProtocol.genShareDelta
// (dckks/keyswitching.go:69-94, dbfv/keyswitching.go:81-109) does in front of its ModDown, the last line of PCKSProtocol.GenShare
// (dckks/public_keyswitching.go:90), and AggregateShares / KeySwitch of all four protocols as one n-ary fold.  Streaming passes
// (lr_stream.hpp), batch on blockIdx.z.  The noise and the ternary u are expanded by launch_ckks_expand, launch_bfv_ternary and
// launch_bfv_noise.
#include "lr_stream.hpp"

namespace lr {

// Sub (:64), MulCoeffsMontgomeryLvl (:74), MulScalarBigintLvl (:76) and AddLvl (:80) of dckks/keyswitching.go on one row of Q: 4 rows read
// (c1, sk_in, sk_out, the transformed noise), one written.  Sub is CRed((a + q) - b): equal keys give CRed(q) = 0.
template <bool ADDEND>
__global__ __launch_bounds__(256) void cks_share_kernel(CksShareLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const u64 q = lp.q, pm = L.pmont.v[limb];
    const long long row = (long long)limb * L.n;
    const ulonglong2 *pc = row_in(L.c1, b, L.c1_stride, row);
    const ulonglong2 *pi = row_in(L.sk_in, b, L.sk_in_stride, row), *ps = row_in(L.sk_out, b, L.sk_out_stride, row);
    const ulonglong2 *pe = ADDEND ? row_in(L.e, b, L.e_stride, row) : nullptr;
    ulonglong2 *po = row_out(L.out, b, L.out_stride, row);
    const int pairs = L.n >> 1;
    LR_FOR_PAIRS(e, pairs) {
        const ulonglong2 c = ld_stream(pc + e), si = ld_shared(pi, L.sk_in_stride, e), so = ld_shared(ps, L.sk_out_stride, e);
        ulonglong2 x = muls2(mul2(c, sub2(si, so, q), q, lp.qinv), pm, q, lp.qinv);
        if constexpr (ADDEND) x = add2(x, ld_stream(pe + e), q);
        st_stream(po + e, x);
    }
}

hipError_t launch_cks_share(const CksShareLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    const dim3 grid = pair_grid(L.n, (unsigned)limbs, (unsigned)batch);
    return L.e ? launch_kernel(cks_share_kernel<true>, grid, dim3(256), 0, stream, L) : launch_kernel(cks_share_kernel<false>, grid, dim3(256), 0, stream, L);
}

// out0 = CRed(out0 + MRed(c1, sk)): MulCoeffsMontgomeryAndAddLvl (dckks/public_keyswitching.go:90)
__global__ __launch_bounds__(256) void pcks_addend_kernel(PcksAddendLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const long long row = (long long)limb * L.n;
    const ulonglong2 *pc = row_in(L.c1, b, L.c1_stride, row), *ps = row_in(L.sk, b, L.sk_stride, row);
    ulonglong2 *po = row_out(L.out0, b, L.out0_stride, row);
    const int pairs = L.n >> 1;
    LR_FOR_PAIRS(e, pairs) {
        const ulonglong2 c = ld_stream(pc + e), z = ld_stream(po + e), s = ld_shared(ps, L.sk_stride, e);
        st_stream(po + e, muladd2(z, c, s, lp.q, lp.qinv));
    }
}

hipError_t launch_pcks_addend(const PcksAddendLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    return launch_kernel(pcks_addend_kernel, pair_grid(L.n, (unsigned)limbs, (unsigned)batch), dim3(256), 0, stream, L);
}

// AggregateShares over `count` parties and KeySwitch's Add in one pass: count (+ 1) rows read, one written, where a chain of Context.Add
// moves 3 (count - 1) (+ 3).  The additions keep the reference's order, each with its CRed: a share may hold the residue q_j.  Every lane
// reads all its operands before it stores, so out may be base or any share.  The shares' loads do not depend on the running sum: four are
// in flight per lane.
__global__ __launch_bounds__(256) void fold_kernel(FoldLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const u64 q = L.lp[limb].q;
    const long long row = (long long)limb * L.n;
    const ulonglong2 *pb = L.base ? row_in(L.base, b, L.base_stride, row) : nullptr;
    ulonglong2 *po = row_out(L.out, b, L.out_stride, row);
    const int pairs = L.n >> 1, count = L.count;
    LR_FOR_PAIRS(e, pairs) {
        ulonglong2 acc = ld_stream(row_in(L.share[0].base, b, L.share[0].stride, row) + e);
#pragma unroll 4
        for (int k = 1; k < count; ++k) acc = add2(acc, ld_stream(row_in(L.share[k].base, b, L.share[k].stride, row) + e), q);
        if (pb) acc = add2(ld_stream(pb + e), acc, q);
        st_stream(po + e, acc);
    }
}

hipError_t launch_fold(const FoldLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    return launch_kernel(fold_kernel, pair_grid(L.n, (unsigned)limbs, (unsigned)batch), dim3(256), 0, stream, L);
}

}  // namespace lr
