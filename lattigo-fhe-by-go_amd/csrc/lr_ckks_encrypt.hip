// lr_ckks_encrypt.hip -- the kernels of the CKKS encryptor (lr_ckks_encryptor.cpp): the samplers' compact decisions expanded into the polys
// that the forward transform of the fast forms takes, and the fast forms' element passes after it.  Streaming kernels in the manner of
// lr_bfv_encrypt.hip and lr_ewise.hip: 16 B per lane per access to poly data, two coefficients per lane, limb on blockIdx.y (per-modulus
// constants wave-uniform), batch on blockIdx.z, a grid-stride loop over coefficient pairs.  The through-P forms run on launch_mul2,
// launch_bfv_negmul and launch_bfv_noise.
#include "lr_device.hpp"

namespace lr {

namespace {

dim3 pair_grid(int n, unsigned y, unsigned z) {
    int gx = ((n >> 1) + 255) / 256;
    if (gx > 64) gx = 64;
    if (gx < 1) gx = 1;
    return dim3((unsigned)gx, y, z);
}

// the Gaussian sampler's residue (ring/gaussianSampler.go:247) as the transform's operand: sign 1 -> c, sign 0 -> q - c, and the q of
// (0, sign 0) as 0 -- SampleNTT transforms the poly next and Context.NTT ends on a full reduction, so no bit of its result changes
LR_D u64 noise_operand(unsigned byte, u64 q) {
    const u64 c = byte & 127u;
    return (byte & 128u) || c == 0 ? c : q - c;
}

}  // namespace

// grid y = part * limbs + limb.  Part 0 is the ternary poly when the launch has one (pair e holds coefficients 2e and 2e + 1: both bits of
// a plane sit in byte e >> 2 at bit 2 (e & 3)); the parts after it are the noise polys.
__global__ __launch_bounds__(256) void ckks_expand_kernel(CkksExpandLaunch L, int limbs) {
    const int part = blockIdx.y / limbs, limb = blockIdx.y - part * limbs;
    const long long b = blockIdx.z;
    ulonglong2 *po = reinterpret_cast<ulonglong2 *>(L.out + part * L.part_stride + b * L.out_stride + (long long)limb * L.n);
    const int pairs = L.n >> 1;
    if (L.ternary && part == 0) {
        const u64 one = L.one.v[limb], minus_one = L.minus_one.v[limb];
        const long long plane = (long long)(L.n >> 3);
        const unsigned char *pc = L.coeff_bits + b * plane, *ps = L.sign_bits + b * plane;
        for (int e = blockIdx.x * 256 + threadIdx.x; e < pairs; e += gridDim.x * 256) {
            const unsigned sh = (unsigned)(e & 3) * 2;
            const unsigned c = (unsigned)pc[e >> 2] >> sh, s = (unsigned)ps[e >> 2] >> sh;
            const u64 v0 = (c & 1) ? ((s & 1) ? minus_one : one) : 0;
            const u64 v1 = (c & 2) ? ((s & 2) ? minus_one : one) : 0;
            st_stream(po + e, make_ulonglong2(v0, v1));
        }
        return;
    }
    const u64 q = L.lp[limb].q;
    const unsigned char *pe = L.e[part - L.ternary] + b * (long long)L.n;   // (byte loads: a caller's device pointer may have any alignment)
    for (int e = blockIdx.x * 256 + threadIdx.x; e < pairs; e += gridDim.x * 256)
        st_stream(po + e, make_ulonglong2(noise_operand(pe[2 * e], q), noise_operand(pe[2 * e + 1], q)));
}

hipError_t launch_ckks_expand(const CkksExpandLaunch &L, int limbs, int batch, hipStream_t stream) {
    const int parts = L.ternary + L.noises;
    if (limbs <= 0 || batch <= 0 || parts <= 0) return hipSuccess;
    if (L.n < 8 || limbs > kMaxLimbs || L.ternary < 0 || L.ternary > 1 || L.noises < 0 || L.noises > 2 || batch > 65535)
        return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(ckks_expand_kernel, pair_grid(L.n, (unsigned)(parts * limbs), (unsigned)batch), dim3(256), 0, stream, L, limbs);
    return hipGetLastError();
}

// ct_k = CRed(MRed(u, pk_k) + e_k), then CRed(ct_0 + pt): ckks/encryptor.go:190-200, :234 with every operand read once
__global__ __launch_bounds__(256) void ckks_pk_fast_kernel(CkksPkFastLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const u64 q = lp.q;
    const long long row = (long long)limb * L.n;
    const ulonglong2 *pu = reinterpret_cast<const ulonglong2 *>(L.u + b * L.r_stride + row);
    const ulonglong2 *pe0 = reinterpret_cast<const ulonglong2 *>(L.e0 + b * L.r_stride + row);
    const ulonglong2 *pe1 = reinterpret_cast<const ulonglong2 *>(L.e1 + b * L.r_stride + row);
    const ulonglong2 *pk0 = reinterpret_cast<const ulonglong2 *>(L.pk0 + b * L.pk0_stride + row);
    const ulonglong2 *pk1 = reinterpret_cast<const ulonglong2 *>(L.pk1 + b * L.pk1_stride + row);
    const ulonglong2 *pp = reinterpret_cast<const ulonglong2 *>(L.pt + b * L.pt_stride + row);
    ulonglong2 *po0 = reinterpret_cast<ulonglong2 *>(L.out0 + b * L.out0_stride + row);
    ulonglong2 *po1 = reinterpret_cast<ulonglong2 *>(L.out1 + b * L.out1_stride + row);
    const int pairs = L.n >> 1;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < pairs; e += gridDim.x * 256) {
        const ulonglong2 u = ld_stream(pu + e), e0 = ld_stream(pe0 + e), e1 = ld_stream(pe1 + e);
        const ulonglong2 k0 = L.pk0_stride ? ld_stream(pk0 + e) : pk0[e];     // (a key shared by the batch: through the caches)
        const ulonglong2 k1 = L.pk1_stride ? ld_stream(pk1 + e) : pk1[e];
        const ulonglong2 p = L.pt_stride ? ld_stream(pp + e) : pp[e];
        ulonglong2 c0, c1;
        c0.x = cred(cred(mred(u.x, k0.x, q, lp.qinv) + e0.x, q) + p.x, q);
        c0.y = cred(cred(mred(u.y, k0.y, q, lp.qinv) + e0.y, q) + p.y, q);
        c1.x = cred(mred(u.x, k1.x, q, lp.qinv) + e1.x, q);
        c1.y = cred(mred(u.y, k1.y, q, lp.qinv) + e1.y, q);
        st_stream(po0 + e, c0);
        st_stream(po1 + e, c1);
    }
}

hipError_t launch_ckks_pk_fast(const CkksPkFastLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (limbs <= 0 || batch <= 0) return hipSuccess;
    if (L.n < 2 || batch > 65535) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(ckks_pk_fast_kernel, pair_grid(L.n, (unsigned)limbs, (unsigned)batch), dim3(256), 0, stream, L);
    return hipGetLastError();
}

// ct0 = CRed(CRed((q - MRed(crp, sk)) + e) + pt), ct1 = crp: ckks/encryptor.go:324-330, :359.  The negation keeps the reference's q for a
// zero product, the one value of the chain that is not a canonical residue.
__global__ __launch_bounds__(256) void ckks_sk_fast_kernel(CkksSkFastLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const u64 q = lp.q;
    const long long row = (long long)limb * L.n;
    const ulonglong2 *pa = reinterpret_cast<const ulonglong2 *>(L.crp + b * L.crp_stride + row);
    const ulonglong2 *ps = reinterpret_cast<const ulonglong2 *>(L.sk + b * L.sk_stride + row);
    const ulonglong2 *pe = reinterpret_cast<const ulonglong2 *>(L.e + b * L.e_stride + row);
    const ulonglong2 *pp = reinterpret_cast<const ulonglong2 *>(L.pt + b * L.pt_stride + row);
    ulonglong2 *po0 = reinterpret_cast<ulonglong2 *>(L.out0 + b * L.out0_stride + row);
    ulonglong2 *po1 = reinterpret_cast<ulonglong2 *>(L.out1 + b * L.out1_stride + row);
    const int pairs = L.n >> 1;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < pairs; e += gridDim.x * 256) {
        const ulonglong2 a = ld_stream(pa + e), x = ld_stream(pe + e);
        const ulonglong2 s = L.sk_stride ? ld_stream(ps + e) : ps[e];
        const ulonglong2 p = L.pt_stride ? ld_stream(pp + e) : pp[e];
        ulonglong2 c0;
        c0.x = cred(cred((q - mred(a.x, s.x, q, lp.qinv)) + x.x, q) + p.x, q);
        c0.y = cred(cred((q - mred(a.y, s.y, q, lp.qinv)) + x.y, q) + p.y, q);
        st_stream(po0 + e, c0);
        st_stream(po1 + e, a);
    }
}

hipError_t launch_ckks_sk_fast(const CkksSkFastLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (limbs <= 0 || batch <= 0) return hipSuccess;
    if (L.n < 2 || batch > 65535) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(ckks_sk_fast_kernel, pair_grid(L.n, (unsigned)limbs, (unsigned)batch), dim3(256), 0, stream, L);
    return hipGetLastError();
}

}  // namespace lr
