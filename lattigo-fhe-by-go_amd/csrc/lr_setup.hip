// lr_setup.hip -- the kernels of collective key setup (lr_setup.cpp): what CKGProtocol.GenShare (dbfv/publickey_gen.go:54-57), the three
// rounds of RKGProtocol (dbfv/relinkey_gen.go:215-355), the two of RKGProtocolNaive (dbfv/relinkey_gen_naive.go:59-200) and
// RTGProtocol.genShare / Finalize (dbfv/rotkey_gen.go:139-215) do behind the forward transform of their samples; the dckks twins compute
// the same lines.  Streaming passes (lr_stream.hpp), party x digit on blockIdx.z.  The noise and the ternary polys are expanded by
// launch_ckks_expand; AggregateShare* is launch_fold.
#include "lr_stream.hpp"

namespace lr {

__global__ __launch_bounds__(256) void setup_ckg_kernel(SetupCkgLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const u64 q = lp.q;
    const long long row = (long long)limb * L.n;
    const ulonglong2 *ps = row_in(L.sk, b, L.sk_stride, row), *pa = row_in(L.crs, b, L.crs_stride, row);
    ulonglong2 *po = row_out(L.share, b, L.share_stride, row);
    const int pairs = L.n >> 1;
    LR_FOR_PAIRS(e, pairs) {
        const ulonglong2 v = ld_stream(po + e), s = ld_shared(ps, L.sk_stride, e), a = ld_shared(pa, L.crs_stride, e);
        st_stream(po + e, mulsub2(v, s, a, q, lp.qinv));
    }
}

hipError_t launch_setup_ckg(const SetupCkgLaunch &L, int rows, int batch, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, rows, batch)) return verdict_error(v);
    return launch_kernel(setup_ckg_kernel, pair_grid(L.n, (unsigned)rows, (unsigned)batch), dim3(256), 0, stream, L);
}

// One share kernel per protocol step, z = party * beta + digit, what follows the transform in one pass:
//   kSetupRkg1   (dbfv/relinkey_gen.go:229-254)  x = e; own rows: x = CRed(x + skP); out[digit] = CRed(x + (q - MRed(u, crp[digit])))
//   kSetupRkg2   (:281-297)  out[2 digit] = CRed(MRed(round1[digit], sk) + e1), out[2 digit + 1] = CRed(e2 + MRed(sk, crp[digit])): both
//                from one read of sk
//   kSetupRkg3   (:325-332)  out[digit] = CRed(e + MRed(CRed((u + q) - sk), round2[2 digit + 1])): u - sk stays in registers
//   kSetupNaive1 (dbfv/relinkey_gen_naive.go:71-107)  x0 = e0 (dckks: e1, its :73-75), own rows: x0 = CRed(x0 + skP);
//                out[2 digit] = CRed(x0 + MRed(pk0, t)), out[2 digit + 1] = CRed(e1 + MRed(pk1, t)) (dckks: MRed(pk1, t), onto a zero share)
//   kSetupNaive2 (:139-163)  out[2 digit + c] = CRed(CRed(MRed(round1[2 digit + c], sk) + MRed(pk_c, t)) + e_c)
//   kSetupRtg    (dbfv/rotkey_gen.go:143-181)  z = key * beta + digit: x = e; own rows: x = CRed(x + (PermuteNTT(sk, gen) times P));
//                out[digit] = MForm(CRed(x + (q - MRed(crp[digit], sk)))): the Galois gather of sk inside the pass
template <int KIND>
__global__ __launch_bounds__(256) void setup_share_kernel(SetupShareLaunch L) {
    constexpr bool PAIR_OUT = KIND == kSetupRkg2 || KIND == kSetupNaive1 || KIND == kSetupNaive2;
    constexpr int PER = PAIR_OUT ? 2 : 1;
    const int limb = blockIdx.y;
    const int k = blockIdx.z / L.beta, digit = blockIdx.z - k * L.beta;
    const LimbParams lp = L.lp[limb];
    const u64 q = lp.q, qinv = lp.qinv;
    const long long row = (long long)limb * L.n, z = blockIdx.z;
    const bool own = limb >= digit * L.alpha && limb < (digit + 1) * L.alpha && limb < L.nQ;     // the digit loop with its break
    const u64 pm = own ? L.pmont.v[limb] : 0;
    const KeygenKeyRef ref = L.out[k];
    const ulonglong2 *pe = row_in(L.e, z * PER, L.e_stride, row), *pe1 = row_in(L.e, z * PER + 1, L.e_stride, row);
    const u64 *sk = L.sk + (KIND == kSetupRtg ? 0 : (long long)k * L.sk_stride) + row;
    const ulonglong2 *ps = reinterpret_cast<const ulonglong2 *>(sk);
    ulonglong2 *po = row_out(ref.base, PER * digit, ref.stride, row), *po1 = row_out(ref.base, PER * digit + 1, ref.stride, row);
    const ulonglong2 *pu = nullptr, *pa = nullptr, *pin = nullptr, *pin1 = nullptr, *pt = nullptr, *pk0 = nullptr, *pk1 = nullptr;
    if constexpr (KIND == kSetupRkg1 || KIND == kSetupRkg3) pu = row_in(L.u, k, L.u_stride, row);
    if constexpr (KIND == kSetupRkg1 || KIND == kSetupRkg2 || KIND == kSetupRtg) pa = row_in(L.crp, digit, L.crp_stride, row);
    if constexpr (KIND == kSetupRkg2) pin = row_in(L.in, digit, L.in_stride, row);
    if constexpr (KIND == kSetupRkg3) pin = row_in(L.in, 2 * digit + 1, L.in_stride, row);
    if constexpr (KIND == kSetupNaive2) {
        pin = row_in(L.in, 2 * digit, L.in_stride, row);
        pin1 = row_in(L.in, 2 * digit + 1, L.in_stride, row);
    }
    if constexpr (KIND == kSetupNaive1 || KIND == kSetupNaive2) {
        pt = row_in(L.t, z, L.t_stride, row);
        pk0 = row_in(L.pk0, 0, 0, row);
        pk1 = row_in(L.pk1, 0, 0, row);
    }
    const u32 gen = KIND == kSetupRtg ? L.gen[k] : 1u, mask2 = 2u * (u32)L.n - 1u;
    const int pairs = L.n >> 1, logn = L.logn;
    LR_FOR_PAIRS(e, pairs) {
        ulonglong2 x = ld_stream(pe + e);
        if constexpr (KIND == kSetupRkg1) {
            const ulonglong2 u = pu[e], a = pa[e];                            // (shared by the digits or the parties: through the caches)
            if (own) {
                const ulonglong2 s = ps[e];
                x = add2(x, times_p2(s.x, s.y, pm, q, qinv), q);
            }
            st_stream(po + e, mulsub2(x, u, a, q, qinv));
        } else if constexpr (KIND == kSetupRkg2) {
            const ulonglong2 s = ps[e], a = pa[e], r = pin[e], e2 = ld_stream(pe1 + e);
            st_stream(po + e, add2(mul2(r, s, q, qinv), x, q));
            st_stream(po1 + e, add2(e2, mul2(s, a, q, qinv), q));
        } else if constexpr (KIND == kSetupRkg3) {
            const ulonglong2 s = ps[e], u = pu[e], r = pin[e];
            st_stream(po + e, add2(x, mul2(sub2(u, s, q), r, q, qinv), q));
        } else if constexpr (KIND == kSetupNaive1) {
            const ulonglong2 t = ld_stream(pt + e), e1 = ld_stream(pe1 + e), p0 = pk0[e], p1 = pk1[e];
            ulonglong2 x0 = L.quirk ? e1 : x;
            if (own) {
                const ulonglong2 s = ps[e];
                x0 = add2(x0, times_p2(s.x, s.y, pm, q, qinv), q);
            }
            st_stream(po + e, add2(x0, mul2(p0, t, q, qinv), q));
            st_stream(po1 + e, add2(L.quirk ? make_ulonglong2(0, 0) : e1, mul2(p1, t, q, qinv), q));
        } else if constexpr (KIND == kSetupNaive2) {
            const ulonglong2 t = ld_stream(pt + e), e1 = ld_stream(pe1 + e), p0 = pk0[e], p1 = pk1[e], s = ps[e], r0 = pin[e], r1 = pin1[e];
            st_stream(po + e, add2(add2(mul2(r0, s, q, qinv), mul2(p0, t, q, qinv), q), x, q));
            st_stream(po1 + e, add2(add2(mul2(r1, s, q, qinv), mul2(p1, t, q, qinv), q), e1, q));
        } else {
            const ulonglong2 s = ps[e], a = pa[e];
            if (own) {
                const u64 g0 = sk[galois_index(2u * (u32)e, gen, mask2, logn)], g1 = sk[galois_index(2u * (u32)e + 1u, gen, mask2, logn)];
                x = add2(x, times_p2(g0, g1, pm, q, qinv), q);
            }
            st_stream(po + e, mform2(mulsub2(x, a, s, q, qinv), lp));
        }
    }
}

hipError_t launch_setup_share(int kind, const SetupShareLaunch &L, int rows, int parties, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, rows, parties)) return verdict_error(v);
    const dim3 grid = pair_grid(L.n, (unsigned)rows, (unsigned)(parties * L.beta));
    switch (kind) {
        case kSetupRkg1: return launch_kernel(setup_share_kernel<kSetupRkg1>, grid, dim3(256), 0, stream, L);
        case kSetupRkg2: return launch_kernel(setup_share_kernel<kSetupRkg2>, grid, dim3(256), 0, stream, L);
        case kSetupRkg3: return launch_kernel(setup_share_kernel<kSetupRkg3>, grid, dim3(256), 0, stream, L);
        case kSetupNaive1: return launch_kernel(setup_share_kernel<kSetupNaive1>, grid, dim3(256), 0, stream, L);
        case kSetupNaive2: return launch_kernel(setup_share_kernel<kSetupNaive2>, grid, dim3(256), 0, stream, L);
        case kSetupRtg: return launch_kernel(setup_share_kernel<kSetupRtg>, grid, dim3(256), 0, stream, L);
        default: return hipErrorInvalidValue;
    }
}

__global__ __launch_bounds__(256) void setup_key_kernel(SetupKeyLaunch L) {
    const int limb = blockIdx.y;
    const long long i = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const long long row = (long long)limb * L.n;
    ulonglong2 *po0 = row_out(L.key, 2 * i, L.key_stride, row), *po1 = row_out(L.key, 2 * i + 1, L.key_stride, row);
    const ulonglong2 *pp0 = L.pairs ? row_in(L.pairs, 2 * i, L.pairs_stride, row) : nullptr;
    const ulonglong2 *pp1 = L.pairs ? row_in(L.pairs, 2 * i + 1, L.pairs_stride, row) : nullptr;
    const ulonglong2 *pv = L.polys ? row_in(L.polys, i, L.polys_stride, row) : nullptr;
    const ulonglong2 *pa = L.crp ? row_in(L.crp, i, L.crp_stride, row) : nullptr;
    const int pairs = L.n >> 1;
    LR_FOR_PAIRS(e, pairs) {
        if (pp0) {
            ulonglong2 x = ld_stream(pp0 + e);
            const ulonglong2 y = ld_stream(pp1 + e);
            if (pv) x = add2(x, ld_stream(pv + e), lp.q);
            st_stream(po0 + e, mform2(x, lp));
            st_stream(po1 + e, mform2(y, lp));
        } else {
            st_stream(po0 + e, ld_stream(pv + e));
            st_stream(po1 + e, mform2(ld_stream(pa + e), lp));
        }
    }
}

hipError_t launch_setup_key(const SetupKeyLaunch &L, int rows, int beta, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, rows, beta)) return verdict_error(v);
    return launch_kernel(setup_key_kernel, pair_grid(L.n, (unsigned)rows, (unsigned)beta), dim3(256), 0, stream, L);
}

}  // namespace lr
