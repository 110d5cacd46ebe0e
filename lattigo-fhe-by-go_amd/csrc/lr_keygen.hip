// lr_keygen.hip -- the kernels of the key generator (lr_keygen.cpp): what newSwitchingKey (ckks/keygen.go:282-338, bfv/keygen.go:285-333)
// and GenPublicKey (ckks/keygen.go:138-151) do around the forward transform of the sampled noise.  Streaming kernels in the manner of
// lr_ckks_encrypt.hip: 16 B per lane per access to poly data, two coefficients per lane, limb on blockIdx.y (per-modulus constants
// wave-uniform), key or key x digit on blockIdx.z, a grid-stride loop over coefficient pairs.  The noise and the ternary secret are
// expanded by launch_ckks_expand.
#include "lr_device.hpp"

namespace lr {

namespace {

dim3 pair_grid(int n, unsigned y, unsigned z) {
    int gx = ((n >> 1) + 255) / 256;
    if (gx > 64) gx = 64;
    if (gx < 1) gx = 1;
    return dim3((unsigned)gx, y, z);
}

// ring.PermuteNTTIndex (ring/ring_galois.go:29-52) for one position, as permute_kernel computes it
LR_D u32 galois_index(u32 j, u32 gen, u32 mask2, int logn) {
    const u32 t1 = 2 * (__brev(j) >> (32 - logn)) + 1;
    const u32 t2 = (((gen * t1) & mask2) - 1) >> 1;
    return __brev(t2) >> (32 - logn);
}

}  // namespace

// skIn of key z over the rows of Q: PermuteNTT(sk, gen_z) (genrotKey, ckks/keygen.go:489) and MulScalarBigint by P (:290) in one pass,
// out = MRed(sk[index(j)], MForm(P mod q)).  gen = 1 is the identity gather: GenSwitchingKey's copy (:254).
__global__ __launch_bounds__(256) void keygen_skin_kernel(KeygenSkInLaunch L) {
    const int limb = blockIdx.y;
    const long long k = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const u64 pm = L.pmont.v[limb];
    const u64 *ps = L.sk + k * L.sk_stride + (long long)limb * L.n;
    ulonglong2 *po = reinterpret_cast<ulonglong2 *>(L.out + k * L.out_stride + (long long)limb * L.n);
    const u32 gen = L.gen[k], mask2 = 2u * (u32)L.n - 1u;
    const int pairs = L.n >> 1, logn = L.logn;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < pairs; e += gridDim.x * 256) {
        const u64 x0 = ps[galois_index(2u * (u32)e, gen, mask2, logn)], x1 = ps[galois_index(2u * (u32)e + 1u, gen, mask2, logn)];
        st_stream(po + e, make_ulonglong2(mred(x0, pm, lp.q, lp.qinv), mred(x1, pm, lp.q, lp.qinv)));
    }
}

hipError_t launch_keygen_skin(const KeygenSkInLaunch &L, int limbs, int keys, hipStream_t stream) {
    if (limbs <= 0 || keys <= 0) return hipSuccess;
    if (L.n < 2 || L.logn < 1 || L.logn > 30 || (1 << L.logn) != L.n || limbs > kMaxLimbs || keys > kKeygenKeysPerLaunch) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(keygen_skin_kernel, pair_grid(L.n, (unsigned)limbs, (unsigned)keys), dim3(256), 0, stream, L);
    return hipGetLastError();
}

// GenRelinKey's running product (bfv/keygen.go:186-190): x = MRed(sk, MForm(P)), then x = MRed(x, sk) once per power; key k of the launch
// takes the x of power first + k, that is P sk^(first + k + 2).  ckks/keygen.go:199-200, :290 multiplies in the other order: MRed is fully
// reduced, so the residue is the same.
__global__ __launch_bounds__(256) void keygen_powers_kernel(KeygenPowersLaunch L) {
    const int limb = blockIdx.y;
    const LimbParams lp = L.lp[limb];
    const u64 pm = L.pmont.v[limb];
    const long long row = (long long)limb * L.n;
    const ulonglong2 *ps = reinterpret_cast<const ulonglong2 *>(L.sk + row);
    const int pairs = L.n >> 1;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < pairs; e += gridDim.x * 256) {
        const ulonglong2 s = ps[e];
        ulonglong2 x = make_ulonglong2(mred(s.x, pm, lp.q, lp.qinv), mred(s.y, pm, lp.q, lp.qinv));
        for (int p = 0; p < L.first + L.keys; ++p) {
            x.x = mred(x.x, s.x, lp.q, lp.qinv);
            x.y = mred(x.y, s.y, lp.q, lp.qinv);
            if (p >= L.first) st_stream(reinterpret_cast<ulonglong2 *>(L.out + (long long)(p - L.first) * L.out_stride + row) + e, x);
        }
    }
}

hipError_t launch_keygen_powers(const KeygenPowersLaunch &L, int limbs, hipStream_t stream) {
    if (limbs <= 0 || L.keys <= 0) return hipSuccess;
    if (L.n < 2 || limbs > kMaxLimbs || L.first < 0) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(keygen_powers_kernel, pair_grid(L.n, (unsigned)limbs, 1u), dim3(256), 0, stream, L);
    return hipGetLastError();
}

// evakey[i][0] of key k, z = k * beta + i, every row of Q||P (ckks/keygen.go:303-334): x = MForm(NTT(e)); on the rows digit i owns,
// x = CRed(x + P skIn); x = CRed(x + (q - MRed(a, skOut))).  a = evakey[i][1] is read where the caller put it and not written.
__global__ __launch_bounds__(256) void keygen_finish_kernel(KeygenFinishLaunch L) {
    const int limb = blockIdx.y;
    const int k = blockIdx.z / L.beta, digit = blockIdx.z - k * L.beta;
    const LimbParams lp = L.lp[limb];
    const u64 q = lp.q;
    const long long row = (long long)limb * L.n;
    const KeygenKeyRef key = L.key[k];
    const ulonglong2 *pe = reinterpret_cast<const ulonglong2 *>(L.e + (long long)blockIdx.z * L.e_stride + row);
    const ulonglong2 *pa = reinterpret_cast<const ulonglong2 *>(key.base + (long long)(2 * digit + 1) * key.stride + row);
    ulonglong2 *po = reinterpret_cast<ulonglong2 *>(key.base + (long long)(2 * digit) * key.stride + row);
    const ulonglong2 *pso = reinterpret_cast<const ulonglong2 *>(L.skout + (long long)k * L.skout_stride + row);
    const bool own = limb >= digit * L.alpha && limb < (digit + 1) * L.alpha && limb < L.nQ;     // the loop of :315-331 with its break
    const ulonglong2 *psi = own ? reinterpret_cast<const ulonglong2 *>(L.skin + (long long)k * L.skin_stride + row) : nullptr;
    const int pairs = L.n >> 1;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < pairs; e += gridDim.x * 256) {
        const ulonglong2 v = ld_stream(pe + e), a = ld_stream(pa + e), s = pso[e];     // (skOut is shared by the digits: through the caches)
        ulonglong2 x = make_ulonglong2(mform(v.x, q, lp.bred_hi, lp.bred_lo), mform(v.y, q, lp.bred_hi, lp.bred_lo));
        if (own) {
            const ulonglong2 t = psi[e];
            x.x = cred(x.x + t.x, q);
            x.y = cred(x.y + t.y, q);
        }
        x.x = cred(x.x + (q - mred(a.x, s.x, q, lp.qinv)), q);
        x.y = cred(x.y + (q - mred(a.y, s.y, q, lp.qinv)), q);
        st_stream(po + e, x);
    }
}

hipError_t launch_keygen_finish(const KeygenFinishLaunch &L, int rows, int keys, hipStream_t stream) {
    if (rows <= 0 || keys <= 0) return hipSuccess;
    if (L.n < 2 || rows > kMaxLimbs || keys > kKeygenKeysPerLaunch || L.beta < 1 || L.beta > kMaxLimbs || L.alpha < 1 || L.nQ < 1 || L.nQ > rows)
        return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(keygen_finish_kernel, pair_grid(L.n, (unsigned)rows, (unsigned)(keys * L.beta)), dim3(256), 0, stream, L);
    return hipGetLastError();
}

// pk0 = Neg(MulCoeffsMontgomeryAndAdd(sk, pk1, NTT(e))) (ckks/keygen.go:144-148): pk0 holds NTT(e) on entry; q - CRed(e + MRed(sk, pk1)),
// and the Neg of 0 is q as in the reference
__global__ __launch_bounds__(256) void keygen_pk_kernel(KeygenPkLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const u64 q = lp.q;
    const long long row = (long long)limb * L.n;
    const ulonglong2 *ps = reinterpret_cast<const ulonglong2 *>(L.sk + b * L.sk_stride + row);
    const ulonglong2 *pa = reinterpret_cast<const ulonglong2 *>(L.pk1 + b * L.pk1_stride + row);
    ulonglong2 *po = reinterpret_cast<ulonglong2 *>(L.pk0 + b * L.pk0_stride + row);
    const int pairs = L.n >> 1;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < pairs; e += gridDim.x * 256) {
        const ulonglong2 v = ld_stream(po + e), a = ld_stream(pa + e);
        const ulonglong2 s = L.sk_stride ? ld_stream(ps + e) : ps[e];
        st_stream(po + e, make_ulonglong2(q - cred(v.x + mred(s.x, a.x, q, lp.qinv), q), q - cred(v.y + mred(s.y, a.y, q, lp.qinv), q)));
    }
}

hipError_t launch_keygen_pk(const KeygenPkLaunch &L, int rows, int batch, hipStream_t stream) {
    if (rows <= 0 || batch <= 0) return hipSuccess;
    if (L.n < 2 || rows > kMaxLimbs || batch > 65535) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(keygen_pk_kernel, pair_grid(L.n, (unsigned)rows, (unsigned)batch), dim3(256), 0, stream, L);
    return hipGetLastError();
}

}  // namespace lr
