// lr_keygen.hip -- the kernels of the key generator (lr_keygen.cpp): what newSwitchingKey (ckks/keygen.go:282-338, bfv/keygen.go:285-333)
// and GenPublicKey (ckks/keygen.go:138-151) do around the forward transform of the sampled noise.  Streaming passes (lr_stream.hpp), key or
// key x digit on blockIdx.z.  The noise and the ternary secret are expanded by launch_ckks_expand.
#include "lr_stream.hpp"

namespace lr {

// skIn of key z over the rows of Q: PermuteNTT(sk, gen_z) (genrotKey, ckks/keygen.go:489) and MulScalarBigint by P (:290) in one pass,
// out = MRed(sk[index(j)], MForm(P mod q)).  gen = 1 is the identity gather: GenSwitchingKey's copy (:254).
__global__ __launch_bounds__(256) void keygen_skin_kernel(KeygenSkInLaunch L) {
    const int limb = blockIdx.y;
    const long long k = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const u64 pm = L.pmont.v[limb];
    const u64 *ps = L.sk + k * L.sk_stride + (long long)limb * L.n;
    ulonglong2 *po = row_out(L.out, k, L.out_stride, (long long)limb * L.n);
    const u32 gen = L.gen[k], mask2 = 2u * (u32)L.n - 1u;
    const int pairs = L.n >> 1, logn = L.logn;
    LR_FOR_PAIRS(e, pairs) {
        const u64 x0 = ps[galois_index(2u * (u32)e, gen, mask2, logn)], x1 = ps[galois_index(2u * (u32)e + 1u, gen, mask2, logn)];
        st_stream(po + e, muls2(make_ulonglong2(x0, x1), pm, lp.q, lp.qinv));
    }
}

hipError_t launch_keygen_skin(const KeygenSkInLaunch &L, int limbs, int keys, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, keys)) return verdict_error(v);
    return launch_kernel(keygen_skin_kernel, pair_grid(L.n, (unsigned)limbs, (unsigned)keys), dim3(256), 0, stream, L);
}

// GenRelinKey's running product (bfv/keygen.go:186-190): x = MRed(sk, MForm(P)), then x = MRed(x, sk) once per power; key k of the launch
// takes the x of power first + k, that is P sk^(first + k + 2).  ckks/keygen.go:199-200, :290 multiplies in the other order: MRed is fully
// reduced, so the residue is the same.
__global__ __launch_bounds__(256) void keygen_powers_kernel(KeygenPowersLaunch L) {
    const int limb = blockIdx.y;
    const LimbParams lp = L.lp[limb];
    const u64 pm = L.pmont.v[limb];
    const long long row = (long long)limb * L.n;
    const ulonglong2 *ps = row_in(L.sk, 0, 0, row);
    const int pairs = L.n >> 1;
    LR_FOR_PAIRS(e, pairs) {
        const ulonglong2 s = ps[e];
        ulonglong2 x = muls2(s, pm, lp.q, lp.qinv);
        for (int p = 0; p < L.first + L.keys; ++p) {
            x = mul2(x, s, lp.q, lp.qinv);
            if (p >= L.first) st_stream(row_out(L.out, p - L.first, L.out_stride, row) + e, x);
        }
    }
}

hipError_t launch_keygen_powers(const KeygenPowersLaunch &L, int limbs, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, limbs)) return verdict_error(v);
    return launch_kernel(keygen_powers_kernel, pair_grid(L.n, (unsigned)limbs, 1u), dim3(256), 0, stream, L);
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
    const ulonglong2 *pe = row_in(L.e, blockIdx.z, L.e_stride, row);
    const ulonglong2 *pa = row_in(key.base, 2 * digit + 1, key.stride, row);
    ulonglong2 *po = row_out(key.base, 2 * digit, key.stride, row);
    const ulonglong2 *pso = row_in(L.skout, k, L.skout_stride, row);
    const bool own = limb >= digit * L.alpha && limb < (digit + 1) * L.alpha && limb < L.nQ;     // the loop of :315-331 with its break
    const ulonglong2 *psi = own ? row_in(L.skin, k, L.skin_stride, row) : nullptr;
    const int pairs = L.n >> 1;
    LR_FOR_PAIRS(e, pairs) {
        const ulonglong2 v = ld_stream(pe + e), a = ld_stream(pa + e), s = pso[e];     // (skOut is shared by the digits: through the caches)
        ulonglong2 x = mform2(v, lp);
        if (own) x = add2(x, psi[e], q);
        st_stream(po + e, mulsub2(x, a, s, q, lp.qinv));
    }
}

hipError_t launch_keygen_finish(const KeygenFinishLaunch &L, int rows, int keys, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, rows, keys)) return verdict_error(v);
    return launch_kernel(keygen_finish_kernel, pair_grid(L.n, (unsigned)rows, (unsigned)(keys * L.beta)), dim3(256), 0, stream, L);
}

// pk0 = Neg(MulCoeffsMontgomeryAndAdd(sk, pk1, NTT(e))) (ckks/keygen.go:144-148): pk0 holds NTT(e) on entry; q - CRed(e + MRed(sk, pk1)),
// and the Neg of 0 is q as in the reference
__global__ __launch_bounds__(256) void keygen_pk_kernel(KeygenPkLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const u64 q = lp.q;
    const long long row = (long long)limb * L.n;
    const ulonglong2 *ps = row_in(L.sk, b, L.sk_stride, row), *pa = row_in(L.pk1, b, L.pk1_stride, row);
    ulonglong2 *po = row_out(L.pk0, b, L.pk0_stride, row);
    const int pairs = L.n >> 1;
    LR_FOR_PAIRS(e, pairs) {
        const ulonglong2 v = ld_stream(po + e), a = ld_stream(pa + e), s = ld_shared(ps, L.sk_stride, e);
        st_stream(po + e, neg2(muladd2(v, s, a, q, lp.qinv), q));
    }
}

hipError_t launch_keygen_pk(const KeygenPkLaunch &L, int rows, int batch, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, rows, batch)) return verdict_error(v);
    return launch_kernel(keygen_pk_kernel, pair_grid(L.n, (unsigned)rows, (unsigned)batch), dim3(256), 0, stream, L);
}

}  // namespace lr
