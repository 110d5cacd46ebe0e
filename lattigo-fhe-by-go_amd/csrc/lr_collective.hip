// lr_collective.hip -- the kernels of collective key switching (lr_collective.cpp): what CKSProtocol.genShareDelta
// (dckks/keyswitching.go:69-94, dbfv/keyswitching.go:81-109) does in front of its ModDown, the last line of PCKSProtocol.GenShare
// (dckks/public_keyswitching.go:90), and AggregateShares / KeySwitch of all four protocols as one n-ary fold.  Streaming kernels in the
// manner of lr_keygen.hip: 16 B per lane per access to poly data, two coefficients per lane, limb on blockIdx.y (per-modulus constants
// wave-uniform), batch on blockIdx.z, a grid-stride loop over coefficient pairs.  The noise and the ternary u are expanded by
// launch_ckks_expand, launch_bfv_ternary and launch_bfv_noise.
#include "lr_device.hpp"

namespace lr {

namespace {

dim3 pair_grid(int n, unsigned y, unsigned z) {
    int gx = ((n >> 1) + 255) / 256;
    if (gx > 64) gx = 64;
    if (gx < 1) gx = 1;
    return dim3((unsigned)gx, y, z);
}

}  // namespace

// Sub (:64), MulCoeffsMontgomeryLvl (:74), MulScalarBigintLvl (:76) and AddLvl (:80) of dckks/keyswitching.go on one row of Q: 4 rows read
// (c1, sk_in, sk_out, the transformed noise), one written.  Sub is CRed((a + q) - b): equal keys give CRed(q) = 0.
template <bool ADDEND>
__global__ __launch_bounds__(256) void cks_share_kernel(CksShareLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const u64 q = lp.q, pm = L.pmont.v[limb];
    const long long row = (long long)limb * L.n;
    const ulonglong2 *pc = reinterpret_cast<const ulonglong2 *>(L.c1 + b * L.c1_stride + row);
    const ulonglong2 *pi = reinterpret_cast<const ulonglong2 *>(L.sk_in + b * L.sk_in_stride + row);
    const ulonglong2 *ps = reinterpret_cast<const ulonglong2 *>(L.sk_out + b * L.sk_out_stride + row);
    const ulonglong2 *pe = ADDEND ? reinterpret_cast<const ulonglong2 *>(L.e + b * L.e_stride + row) : nullptr;
    ulonglong2 *po = reinterpret_cast<ulonglong2 *>(L.out + b * L.out_stride + row);
    const int pairs = L.n >> 1;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < pairs; e += gridDim.x * 256) {
        const ulonglong2 c = ld_stream(pc + e);
        const ulonglong2 si = L.sk_in_stride ? ld_stream(pi + e) : pi[e];      // (a key shared by the batch: through the caches)
        const ulonglong2 so = L.sk_out_stride ? ld_stream(ps + e) : ps[e];
        ulonglong2 x;
        x.x = mred(mred(c.x, cred((si.x + q) - so.x, q), q, lp.qinv), pm, q, lp.qinv);
        x.y = mred(mred(c.y, cred((si.y + q) - so.y, q), q, lp.qinv), pm, q, lp.qinv);
        if constexpr (ADDEND) {
            const ulonglong2 v = ld_stream(pe + e);
            x.x = cred(x.x + v.x, q);
            x.y = cred(x.y + v.y, q);
        }
        st_stream(po + e, x);
    }
}

hipError_t launch_cks_share(const CksShareLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (limbs <= 0 || batch <= 0) return hipSuccess;
    if (L.n < 2 || limbs > kMaxLimbs || batch > 65535) return hipErrorInvalidValue;
    (void)hipGetLastError();
    const dim3 grid = pair_grid(L.n, (unsigned)limbs, (unsigned)batch);
    if (L.e) hipLaunchKernelGGL(cks_share_kernel<true>, grid, dim3(256), 0, stream, L);
    else hipLaunchKernelGGL(cks_share_kernel<false>, grid, dim3(256), 0, stream, L);
    return hipGetLastError();
}

// out0 = CRed(out0 + MRed(c1, sk)): MulCoeffsMontgomeryAndAddLvl (dckks/public_keyswitching.go:90)
__global__ __launch_bounds__(256) void pcks_addend_kernel(PcksAddendLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const u64 q = lp.q;
    const long long row = (long long)limb * L.n;
    const ulonglong2 *pc = reinterpret_cast<const ulonglong2 *>(L.c1 + b * L.c1_stride + row);
    const ulonglong2 *ps = reinterpret_cast<const ulonglong2 *>(L.sk + b * L.sk_stride + row);
    ulonglong2 *po = reinterpret_cast<ulonglong2 *>(L.out0 + b * L.out0_stride + row);
    const int pairs = L.n >> 1;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < pairs; e += gridDim.x * 256) {
        const ulonglong2 c = ld_stream(pc + e), z = ld_stream(po + e);
        const ulonglong2 s = L.sk_stride ? ld_stream(ps + e) : ps[e];
        st_stream(po + e, make_ulonglong2(cred(z.x + mred(c.x, s.x, q, lp.qinv), q), cred(z.y + mred(c.y, s.y, q, lp.qinv), q)));
    }
}

hipError_t launch_pcks_addend(const PcksAddendLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (limbs <= 0 || batch <= 0) return hipSuccess;
    if (L.n < 2 || limbs > kMaxLimbs || batch > 65535) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(pcks_addend_kernel, pair_grid(L.n, (unsigned)limbs, (unsigned)batch), dim3(256), 0, stream, L);
    return hipGetLastError();
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
    const ulonglong2 *pb = L.base ? reinterpret_cast<const ulonglong2 *>(L.base + b * L.base_stride + row) : nullptr;
    ulonglong2 *po = reinterpret_cast<ulonglong2 *>(L.out + b * L.out_stride + row);
    const int pairs = L.n >> 1, count = L.count;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < pairs; e += gridDim.x * 256) {
        ulonglong2 acc = ld_stream(reinterpret_cast<const ulonglong2 *>(L.share[0].base + b * L.share[0].stride + row) + e);
#pragma unroll 4
        for (int k = 1; k < count; ++k) {
            const ulonglong2 v = ld_stream(reinterpret_cast<const ulonglong2 *>(L.share[k].base + b * L.share[k].stride + row) + e);
            acc.x = cred(acc.x + v.x, q);
            acc.y = cred(acc.y + v.y, q);
        }
        if (pb) {
            const ulonglong2 v = ld_stream(pb + e);
            acc.x = cred(v.x + acc.x, q);
            acc.y = cred(v.y + acc.y, q);
        }
        st_stream(po + e, acc);
    }
}

hipError_t launch_fold(const FoldLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (limbs <= 0 || batch <= 0) return hipSuccess;
    if (L.n < 2 || limbs > kMaxLimbs || batch > 65535 || L.count < 1 || L.count > kFoldSharesPerLaunch) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fold_kernel, pair_grid(L.n, (unsigned)limbs, (unsigned)batch), dim3(256), 0, stream, L);
    return hipGetLastError();
}

}  // namespace lr
