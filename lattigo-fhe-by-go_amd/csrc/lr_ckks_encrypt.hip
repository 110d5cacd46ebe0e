// lr_ckks_encrypt.hip -- the kernels of the CKKS encryptor (lr_ckks_encryptor.cpp): the samplers' compact decisions expanded into the polys
// that the forward transform of the fast forms takes, and the fast forms' element passes after it.  Streaming passes (lr_stream.hpp),
// batch on blockIdx.z.  The through-P forms run on launch_mul2, launch_bfv_negmul and launch_bfv_noise.
#include "lr_stream.hpp"

namespace lr {

// grid y = part * limbs + limb.  Part 0 is the ternary poly when the launch has one; the parts after it are the noise polys, each
// coefficient as the transform's operand (noise_operand).
__global__ __launch_bounds__(256) void ckks_expand_kernel(CkksExpandLaunch L, int limbs) {
    const int part = blockIdx.y / limbs, limb = blockIdx.y - part * limbs;
    const long long b = blockIdx.z;
    ulonglong2 *po = reinterpret_cast<ulonglong2 *>(L.out + part * L.part_stride + b * L.out_stride + (long long)limb * L.n);
    const int pairs = L.n >> 1;
    if (L.ternary && part == 0) {
        const u64 one = L.one.v[limb], minus_one = L.minus_one.v[limb];
        const long long plane = (long long)(L.n >> 3);
        const unsigned char *pc = L.coeff_bits + b * plane, *ps = L.sign_bits + b * plane;
        LR_FOR_PAIRS(e, pairs) st_stream(po + e, ternary_pair(pc, ps, e, one, minus_one));
        return;
    }
    const u64 q = L.lp[limb].q;
    const unsigned char *pe = L.e[part - L.ternary] + b * (long long)L.n;   // (byte loads: a caller's device pointer may have any alignment)
    LR_FOR_PAIRS(e, pairs) st_stream(po + e, make_ulonglong2(noise_operand(pe[2 * e], q), noise_operand(pe[2 * e + 1], q)));
}

hipError_t launch_ckks_expand(const CkksExpandLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    const dim3 grid = pair_grid(L.n, (unsigned)((L.ternary + L.noises) * limbs), (unsigned)batch);
    return launch_kernel(ckks_expand_kernel, grid, dim3(256), 0, stream, L, limbs);
}

// ct_k = CRed(MRed(u, pk_k) + e_k), then CRed(ct_0 + pt): ckks/encryptor.go:190-200, :234 with every operand read once
__global__ __launch_bounds__(256) void ckks_pk_fast_kernel(CkksPkFastLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const u64 q = lp.q;
    const long long row = (long long)limb * L.n;
    const ulonglong2 *pu = row_in(L.u, b, L.r_stride, row), *pe0 = row_in(L.e0, b, L.r_stride, row), *pe1 = row_in(L.e1, b, L.r_stride, row);
    const ulonglong2 *pk0 = row_in(L.pk0, b, L.pk0_stride, row), *pk1 = row_in(L.pk1, b, L.pk1_stride, row);
    const ulonglong2 *pp = row_in(L.pt, b, L.pt_stride, row);
    ulonglong2 *po0 = row_out(L.out0, b, L.out0_stride, row), *po1 = row_out(L.out1, b, L.out1_stride, row);
    const int pairs = L.n >> 1;
    LR_FOR_PAIRS(e, pairs) {
        const ulonglong2 u = ld_stream(pu + e), e0 = ld_stream(pe0 + e), e1 = ld_stream(pe1 + e);
        const ulonglong2 k0 = ld_shared(pk0, L.pk0_stride, e), k1 = ld_shared(pk1, L.pk1_stride, e), p = ld_shared(pp, L.pt_stride, e);
        st_stream(po0 + e, add2(add2(mul2(u, k0, q, lp.qinv), e0, q), p, q));
        st_stream(po1 + e, add2(mul2(u, k1, q, lp.qinv), e1, q));
    }
}

hipError_t launch_ckks_pk_fast(const CkksPkFastLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    return launch_kernel(ckks_pk_fast_kernel, pair_grid(L.n, (unsigned)limbs, (unsigned)batch), dim3(256), 0, stream, L);
}

// ct0 = CRed(CRed((q - MRed(crp, sk)) + e) + pt), ct1 = crp: ckks/encryptor.go:324-330, :359.  The negation keeps the reference's q for a
// zero product, the one value of the chain that is not a canonical residue.
__global__ __launch_bounds__(256) void ckks_sk_fast_kernel(CkksSkFastLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const u64 q = lp.q;
    const long long row = (long long)limb * L.n;
    const ulonglong2 *pa = row_in(L.crp, b, L.crp_stride, row), *ps = row_in(L.sk, b, L.sk_stride, row);
    const ulonglong2 *pe = row_in(L.e, b, L.e_stride, row), *pp = row_in(L.pt, b, L.pt_stride, row);
    ulonglong2 *po0 = row_out(L.out0, b, L.out0_stride, row), *po1 = row_out(L.out1, b, L.out1_stride, row);
    const int pairs = L.n >> 1;
    LR_FOR_PAIRS(e, pairs) {
        const ulonglong2 a = ld_stream(pa + e), x = ld_stream(pe + e);
        const ulonglong2 s = ld_shared(ps, L.sk_stride, e), p = ld_shared(pp, L.pt_stride, e);
        st_stream(po0 + e, add2(add2(neg2(mul2(a, s, q, lp.qinv), q), x, q), p, q));
        st_stream(po1 + e, a);
    }
}

hipError_t launch_ckks_sk_fast(const CkksSkFastLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    return launch_kernel(ckks_sk_fast_kernel, pair_grid(L.n, (unsigned)limbs, (unsigned)batch), dim3(256), 0, stream, L);
}

}  // namespace lr
