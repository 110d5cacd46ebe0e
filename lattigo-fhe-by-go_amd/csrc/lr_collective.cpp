// lr_collective.cpp -- C ABI: lr_collective, the per-ciphertext protocols of dckks and dbfv for a batch of ciphertexts on the device:
// CKSProtocol.GenShare (dckks/keyswitching.go:62-94, dbfv/keyswitching.go:74-109), PCKSProtocol.GenShare
// (dckks/public_keyswitching.go:63-93, dbfv/public_keyswitching.go:111-148) and AggregateShares / KeySwitch of all four as one n-ary fold.
// The randomness arrives in the compact form of the encryptors (lr_bfv_encryptor).  Kernels: lr_collective.hip, the expansions of
// lr_ckks_encrypt.hip and lr_bfv_encrypt.hip, launch_mul2 and launch_ckks_pk_fast where the lines are pkEncryptor.encrypt's.
// The host sanitizer build (tests/host_stub_build.py) compiles this unit with every other; the launchers of lr_collective.hip have their
// stand-in in tests/cpp/hipstub/stub_collective.cpp.  What it shares with the encryptors and lr_keygen.cpp is
// lr_qp_handle.hpp.
#include "lr_qp_handle.hpp"

// what the four New*Protocol constructors build (dckks/keyswitching.go:28-49, dckks/public_keyswitching.go:28-49 and their dbfv twins);
// the contexts, the scalars and the staging of the host-randomness entry points (max_batch * (N / 4 + 2 N) bytes) are QpHandle's
struct lr_collective : lr_host::QpHandle {
    lr_bext *bext = nullptr;                  // NewFastBasisExtender(contextQ, contextP), owned
    u64 *d_pool = nullptr;                    // tmp, share0tmp, share1tmp: three polys over Q||P for max_batch ciphertexts
    u64 *d_zero = nullptr;                    // one poly of zeros over Q||P: the plaintext operand of launch_ckks_pk_fast
    ~lr_collective() {
        for (void *p : {(void *)d_pool, (void *)d_zero})
            if (p) (void)hipFree(p);
        if (bext) lr_bext_destroy(bext);
    }
};

namespace lr_host {
namespace {

// the rows of Q||P a call at `level` reads: limbs 0 .. level of Q and the rows of P; one run of rows at the top level, two below it
struct Span { int row0, count; };
int spans_of(const lr_collective *h, int level, Span s[2]) {
    if (level + 1 == h->nQ) {
        s[0] = Span{0, h->nQ + h->nP};
        return 1;
    }
    s[0] = Span{0, level + 1};
    s[1] = Span{h->nQ, h->nP};
    return 2;
}

// Context.NTT / InvNTT in place on `items` pool polys: limbs 0 .. level under contextQ, the rows of P under contextP
int ntt_rows(lr_collective *h, bool inverse, int level, u64 *p, long long stride, int items) {
    return ntt_qp(h, true, inverse, level + 1, items, p, stride, p, stride);
}

// SampleTernaryMontgomery and / or KYSampler.Sample as the forward transform's operands on the rows a call at `level` reads: `ternary` +
// `noises` parts of `batch` polys from `out` on, part_stride apart
int expand(lr_collective *h, int level, int ternary, const unsigned char *u_coeff, const unsigned char *u_sign, int noises,
           const unsigned char *e0, const unsigned char *e1, u64 *out, long long stride, long long part, int batch) {
    Span s[2];
    const int n_spans = spans_of(h, level, s);
    for (int k = 0; k < n_spans; ++k)
        LR_TRY(expand_qp(h, s[k].row0, s[k].count, ternary, u_coeff, u_sign, noises, e0, e1, out, stride, part, batch));
    return LR_OK;
}

CksShareLaunch share_launch(const lr_collective *h, const u64 *c1, long long c1_stride, const lr_poly *sk_in, const lr_poly *sk_out, const u64 *e,
                            u64 *out, long long stride, int batch) {
    CksShareLaunch S;
    S.c1 = c1; S.c1_stride = c1_stride;
    S.sk_in = sk_in->d; S.sk_in_stride = key_stride(sk_in, batch);
    S.sk_out = sk_out->d; S.sk_out_stride = key_stride(sk_out, batch);
    S.e = e; S.e_stride = stride;
    S.out = out; S.out_stride = stride;
    S.n = (int)h->cQ->h.N;
    S.pmont = h->pmont;
    S.lp = h->d_lp;
    return S;
}

// Sub, MulCoeffsMontgomery and MulScalarBigint of GenShare / genShareDelta in the reference's call-by-call shape: x (NTT domain, limbs
// 0 .. level) -> P x (sk_in - sk_out) in P.p[2], through tmpDelta in P.p[1]
int delta_product(lr_collective *h, int level, const u64 *x, long long x_stride, const lr_poly *sk_in, const lr_poly *sk_out, const Pools &P,
                  int batch) {
    lr_context *cQ = h->cQ;
    LR_TRY(run_ewise(cQ, LR_SUB, h->nQ, batch, sk_in->d, key_stride(sk_in, batch), sk_out->d, key_stride(sk_out, batch), P.p[1], P.stride, nullptr));
    LR_TRY(run_ewise(cQ, LR_MUL_MONT, level + 1, batch, x, x_stride, P.p[1], P.stride, P.p[2], P.stride, nullptr));
    return run_ewise(cQ, LR_MUL_SCALAR_LIMBS, level + 1, batch, P.p[2], P.stride, nullptr, 0, P.p[2], P.stride, &h->pmont);
}

int check_cks(const lr_collective *h, int level, const lr_poly *sk_in, const lr_poly *sk_out, const lr_poly *c1, int batch, const lr_poly *share) {
    LR_TRY(check_call(h, level, batch));
    LR_TRY(h->check_poly(sk_in, h->nQ, batch, true, "the input secret key"));
    LR_TRY(h->check_poly(sk_out, h->nQ, batch, true, "the output secret key"));
    LR_TRY(h->check_poly(c1, level + 1, batch, false, "the ciphertext"));
    LR_TRY(h->check_poly(share, level + 1, batch, false, "the share"));
    const lr_poly *outs[1] = {share}, *ins[3] = {sk_in, sk_out, c1};
    return check_outputs(h, outs, 1, ins, 3);
}

// CKSProtocol.GenShare of dckks (dckks/keyswitching.go:62-94)
int ckks_cks_share(lr_collective *h, int level, const lr_poly *sk_in, const lr_poly *sk_out, const lr_poly *c1, const unsigned char *eb, int batch,
                   lr_poly *share, bool on_device) {
    if (!h || !sk_in || !sk_out || !c1 || !eb || !share) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_cks(h, level, sk_in, sk_out, c1, batch, share));
    LR_HIP(hipSetDevice(h->device));
    if (!on_device) LR_TRY(h->stage_random(&eb, (size_t)batch * (size_t)h->cQ->h.N));
    lr_context *cQ = h->cQ;
    const Pools P = pools_of(h, h->d_pool, batch);
    const int L1 = level + 1;
    const Rows hP{P.p[0], P.stride, h->nQ, 1};
    if (h->call_by_call) {
        LR_TRY(delta_product(h, level, c1->d, c1->stride(), sk_in, sk_out, P, batch));                                // :64, :74, :76
        LR_TRY(expand(h, h->nQ - 1, 0, nullptr, nullptr, 1, eb, nullptr, P.p[0], P.stride, P.part, batch));           // :79 SampleNTT over Q||P
        LR_TRY(ntt_rows(h, false, h->nQ - 1, P.p[0], P.stride, batch));
        LR_TRY(run_ewise(cQ, LR_ADD, L1, batch, P.p[2], P.stride, P.p[0], P.stride, P.p[2], P.stride, nullptr));      // :80
        LR_TRY(run_ntt(h->cP, true, hP, hP, 0, 1, h->nP, batch));                                                     // :90 (ring_basis_extension.go:199-201)
        return moddown_pq_core(h->bext, level, P.p[2], P.stride, hP, batch, share, true);
    }
    // the noise on limbs 0 .. level and on the rows of P; only the rows of Q are transformed: hP is the transformed noise transformed back
    // by ModDownSplitedNTTPQ (ring_basis_extension.go:199-201), that is the noise itself, its q_j of (0, sign 0) reduced to 0
    LR_TRY(expand(h, level, 0, nullptr, nullptr, 1, eb, nullptr, P.p[0], P.stride, P.part, batch));
    LR_TRY(run_ntt(cQ, false, Rows{P.p[0], P.stride, 0, 1}, Rows{P.p[0], P.stride, 0, 1}, 0, 1, L1, batch));
    LR_HIP(launch_cks_share(share_launch(h, c1->d, c1->stride(), sk_in, sk_out, P.p[0], P.p[0], P.stride, batch), L1, batch, cQ->stream));
    return moddown_pq_core(h->bext, level, P.p[0], P.stride, hP, batch, share, true);
}

// CKSProtocol.GenShare of dbfv (dbfv/keyswitching.go:74-109)
int bfv_cks_share(lr_collective *h, const lr_poly *sk_in, const lr_poly *sk_out, const lr_poly *c1, const unsigned char *eb, int batch, lr_poly *share,
                  bool on_device) {
    if (!h || !sk_in || !sk_out || !c1 || !eb || !share) return fail(LR_ERR_ARG, "null argument");
    const int level = h->nQ - 1;
    LR_TRY(check_cks(h, level, sk_in, sk_out, c1, batch, share));
    LR_HIP(hipSetDevice(h->device));
    if (!on_device) LR_TRY(h->stage_random(&eb, (size_t)batch * (size_t)h->cQ->h.N));
    lr_context *cQ = h->cQ;
    const Pools P = pools_of(h, h->d_pool, batch);
    const Rows q0{P.p[0], P.stride, 0, 1}, q2{P.p[2], P.stride, 0, 1};
    LR_TRY(run_ntt(cQ, false, Rows{c1->d, c1->stride(), 0, 1}, q0, 0, 1, h->nQ, batch));                              // :88
    if (h->call_by_call) {
        LR_TRY(delta_product(h, level, P.p[0], P.stride, sk_in, sk_out, P, batch));                                   // :76, :89, :90
        LR_TRY(run_ntt(cQ, true, q2, q2, 0, 1, h->nQ, batch));                                                        // :92
        LR_TRY(noise_qp(h, 0, 1, &eb, &P.p[0], P.stride, h->rows(), batch));                                          // :94 Sample over Q||P
        LR_TRY(run_ewise(cQ, LR_ADD, h->nQ, batch, P.p[2], P.stride, P.p[0], P.stride, P.p[2], P.stride, nullptr));   // :95
        // :97-103: hP = the rows of P as they are, p_j of (0, sign 0) included
        return moddown_pq_core(h->bext, level, P.p[2], P.stride, Rows{P.p[0], P.stride, h->nQ, 1}, batch, share, false);   // :105
    }
    LR_HIP(launch_cks_share(share_launch(h, P.p[0], P.stride, sk_in, sk_out, nullptr, P.p[0], P.stride, batch), h->nQ, batch, cQ->stream));
    LR_TRY(run_ntt(cQ, true, q0, q0, 0, 1, h->nQ, batch));
    LR_TRY(noise_qp(h, 1, 1, &eb, &P.p[0], P.stride, h->nQ, batch));                        // CRed(x + residue) on the rows of Q
    // the residue on the rows of P, p_j written as 0: no bit of the ModDown's output changes (tests/test_oracle_collective.py)
    LR_TRY(expand_qp(h, h->nQ, h->nP, 0, nullptr, nullptr, 1, eb, nullptr, P.p[0], P.stride, 0, batch));
    return moddown_pq_core(h->bext, level, P.p[0], P.stride, Rows{P.p[0], P.stride, h->nQ, 1}, batch, share, false);
}

int check_pcks(const lr_collective *h, int level, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1, const lr_poly *c1, int batch,
               const lr_poly *o0, const lr_poly *o1) {
    LR_TRY(check_call(h, level, batch));
    LR_TRY(h->check_poly(sk, h->nQ, batch, true, "the secret key"));
    LR_TRY(h->check_poly(pk0, h->nQ + h->nP, batch, true, "the public key"));
    LR_TRY(h->check_poly(pk1, h->nQ + h->nP, batch, true, "the public key"));
    LR_TRY(h->check_poly(c1, level + 1, batch, false, "the ciphertext"));
    LR_TRY(h->check_poly(o0, level + 1, batch, false, "the share"));
    LR_TRY(h->check_poly(o1, level + 1, batch, false, "the share"));
    const lr_poly *outs[2] = {o0, o1}, *ins[4] = {sk, pk0, pk1, c1};
    return check_outputs(h, outs, 2, ins, 4);
}

// SampleTernaryMontgomeryNTT over Q||P (dckks/public_keyswitching.go:68, dbfv :116) into P.p[2]
int ternary_ntt(lr_collective *h, const PkRandom &R, const Pools &P, int batch) {
    LR_TRY(ternary_qp(h, P, R.u_coeff, R.u_sign, h->rows(), batch));
    return ntt_rows(h, false, h->nQ - 1, P.p[2], P.stride, batch);
}

// PCKSProtocol.GenShare of dckks (dckks/public_keyswitching.go:63-93)
int ckks_pcks_share(lr_collective *h, int level, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1, const lr_poly *c1, PkRandom R, int batch,
                    lr_poly *o0, lr_poly *o1, bool on_device) {
    if (!h || !sk || !pk0 || !pk1 || !c1 || !R.u_coeff || !R.u_sign || !R.e0 || !R.e1 || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_pcks(h, level, sk, pk0, pk1, c1, batch, o0, o1));
    LR_HIP(hipSetDevice(h->device));
    if (!on_device) LR_TRY(h->stage_random(&R, batch));
    lr_context *cQ = h->cQ;
    const Pools P = pools_of(h, h->d_pool, batch);
    const long long n = (long long)cQ->h.N;
    const int L1 = level + 1, top = h->nQ - 1;
    const lr_poly *pk[2] = {pk0, pk1};
    lr_poly *outs[2] = {o0, o1};
    if (h->call_by_call) {
        const unsigned char *eb[2] = {R.e0, R.e1};
        LR_TRY(ternary_ntt(h, R, P, batch));                                                                          // :68
        for (int k = 0; k < 2; ++k)                                                                                   // :71, :73
            LR_TRY(ewise_qp(h, true, LR_MUL_MONT, batch, P.p[2], P.stride, pk[k]->d, key_stride(pk[k], batch), P.p[k], P.stride));
        for (int k = 0; k < 2; ++k) {                                                                                 // :76-80
            LR_TRY(expand(h, top, 0, nullptr, nullptr, 1, eb[k], nullptr, P.p[2], P.stride, P.part, batch));
            LR_TRY(ntt_rows(h, false, top, P.p[2], P.stride, batch));
            LR_TRY(ewise_qp(h, true, LR_ADD, batch, P.p[k], P.stride, P.p[2], P.stride, P.p[k], P.stride));
        }
        for (int k = 0; k < 2; ++k) {                                                                                 // :83, :87 ModDownNTTPQ
            const Rows pP{P.p[k], P.stride, h->nQ, 1};
            LR_TRY(run_ntt(h->cP, true, pP, pP, 0, 1, h->nP, batch));
            LR_TRY(moddown_pq_core(h->bext, level, P.p[k], P.stride, pP, batch, outs[k], true));
        }
        return run_ewise(cQ, LR_MUL_MONT_AND_ADD, L1, batch, c1->d, c1->stride(), sk->d, key_stride(sk, batch), o0->d, o0->stride(), nullptr);   // :90
    }
    // u, e0, e1 expanded side by side on the rows the ModDowns read, one transform over all three, one pass for both products and sums
    LR_TRY(expand(h, level, 1, R.u_coeff, R.u_sign, 2, R.e0, R.e1, P.p[0], P.stride, P.part, batch));
    LR_TRY(ntt_rows(h, false, level, P.p[0], P.stride, 3 * batch));
    Span s[2];
    const int n_spans = spans_of(h, level, s);
    for (int k = 0; k < n_spans; ++k) {
        const long long off = (long long)s[k].row0 * n;
        CkksPkFastLaunch F;
        F.u = P.p[0] + off; F.e0 = P.p[1] + off; F.e1 = P.p[2] + off;
        F.r_stride = P.stride;
        F.pk0 = pk0->d + off; F.pk0_stride = key_stride(pk0, batch);
        F.pk1 = pk1->d + off; F.pk1_stride = key_stride(pk1, batch);
        F.pt = h->d_zero; F.pt_stride = 0;
        F.out0 = P.p[1] + off; F.out1 = P.p[2] + off;
        F.out0_stride = F.out1_stride = P.stride;
        F.n = (int)n;
        F.lp = h->d_lp + s[k].row0;
        LR_HIP(launch_ckks_pk_fast(F, s[k].count, batch, cQ->stream));
    }
    {   // the rows of P of both sums back in one launch: the two pools are back to back
        const Rows pP{P.p[1], P.stride, h->nQ, 1};
        LR_TRY(run_ntt(h->cP, true, pP, pP, 0, 1, h->nP, 2 * batch));
    }
    for (int k = 0; k < 2; ++k)
        LR_TRY(moddown_pq_core(h->bext, level, P.p[1 + k], P.stride, Rows{P.p[1 + k], P.stride, h->nQ, 1}, batch, outs[k], true));
    PcksAddendLaunch A;
    A.c1 = c1->d; A.c1_stride = c1->stride();
    A.sk = sk->d; A.sk_stride = key_stride(sk, batch);
    A.out0 = o0->d; A.out0_stride = o0->stride();
    A.n = (int)n;
    A.lp = h->d_lp;
    LR_HIP(launch_pcks_addend(A, L1, batch, cQ->stream));
    return LR_OK;
}

// PCKSProtocol.GenShare of dbfv (dbfv/public_keyswitching.go:111-148): pkEncryptor.encrypt's steps through P, then s c1
int bfv_pcks_share(lr_collective *h, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1, const lr_poly *c1, PkRandom R, int batch, lr_poly *o0,
                   lr_poly *o1, bool on_device) {
    if (!h || !sk || !pk0 || !pk1 || !c1 || !R.u_coeff || !R.u_sign || !R.e0 || !R.e1 || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    const int level = h->nQ - 1, rows = h->nQ + h->nP;
    LR_TRY(check_pcks(h, level, sk, pk0, pk1, c1, batch, o0, o1));
    LR_HIP(hipSetDevice(h->device));
    if (!on_device) LR_TRY(h->stage_random(&R, batch));
    lr_context *cQ = h->cQ;
    const Pools P = pools_of(h, h->d_pool, batch);
    const lr_poly *pk[2] = {pk0, pk1};
    lr_poly *outs[2] = {o0, o1};
    const unsigned char *eb[2] = {R.e0, R.e1};
    LR_TRY(ternary_ntt(h, R, P, batch));                                                                              // :116
    if (h->call_by_call) {
        for (int k = 0; k < 2; ++k)                                                                                   // :119, :121
            LR_TRY(ewise_qp(h, true, LR_MUL_MONT, batch, P.p[2], P.stride, pk[k]->d, key_stride(pk[k], batch), P.p[k], P.stride));
        for (int k = 0; k < 2; ++k) LR_TRY(ntt_rows(h, true, level, P.p[k], P.stride, batch));                        // :123-124
        for (int k = 0; k < 2; ++k) {                                                                                 // :127, :129: the residues as a poly, then Context.Add
            LR_TRY(noise_qp(h, 0, 1, &eb[k], &P.p[2], P.stride, rows, batch));
            LR_TRY(ewise_qp(h, true, LR_ADD, batch, P.p[k], P.stride, P.p[2], P.stride, P.p[k], P.stride));
        }
    } else {
        LR_TRY(mul2_qp(h, P, pk0, pk1, rows, batch));
        LR_TRY(ntt_rows(h, true, level, P.p[0], P.stride, 2 * batch));                      // the two pools are back to back
        LR_TRY(noise_qp(h, 1, 2, eb, P.p, P.stride, rows, batch));
    }
    for (int k = 0; k < 2; ++k)                                                                                       // :132, :136
        LR_TRY(moddown_pq_core(h->bext, level, P.p[k], P.stride, Rows{P.p[k], P.stride, h->nQ, 1}, batch, outs[k], false));
    const Rows q2{P.p[2], P.stride, 0, 1};
    LR_TRY(run_ntt(cQ, false, Rows{c1->d, c1->stride(), 0, 1}, q2, 0, 1, h->nQ, batch));                              // :139
    LR_TRY(run_ewise(cQ, LR_MUL_MONT, h->nQ, batch, P.p[2], P.stride, sk->d, key_stride(sk, batch), P.p[2], P.stride, nullptr));   // :140
    LR_TRY(run_ntt(cQ, true, q2, q2, 0, 1, h->nQ, batch));                                                            // :141
    return run_ewise(cQ, LR_ADD, h->nQ, batch, o0->d, o0->stride(), P.p[2], P.stride, o0->d, o0->stride(), nullptr);  // :144
}

}  // namespace
}  // namespace lr_host

extern "C" int lr_collective_create(lr_context *cQ, lr_context *cP, int max_batch, lr_collective **out) {
    return lr_collective_create_ex(cQ, cP, max_batch, nullptr, out);
}

extern "C" int lr_collective_create_ex(lr_context *cQ, lr_context *cP, int max_batch, const lr_options *options, lr_collective **out) {
    return guarded([&]() -> int {
    if (!cQ || !out) return fail(LR_ERR_ARG, "null argument");
    *out = nullptr;
    const char *name = "collective";
    if (!cP) return fail(LR_ERR_ARG, "collective: modulus P is empty (all four protocols divide by P)");
    Options parsed;
    LR_TRY(check_create(name, cQ, max_batch, options, &parsed));
    LR_TRY(check_pair(cQ, cP));
    LR_TRY(same_stream(cQ, cP));
    std::unique_ptr<lr_collective> h(new lr_collective());
    LR_TRY(h->init(name, cQ, cP, max_batch, parsed));
    LR_HIP(hipSetDevice(cQ->device));
    LR_TRY(lr_bext_create(cQ, cP, &h->bext));
    const size_t N = (size_t)cQ->h.N, poly_bytes = (size_t)h->rows() * N * sizeof(u64);
    LR_TRY(h->allocate((size_t)max_batch * (N / 4 + 2 * N)));
    LR_HIP(hipMalloc((void **)&h->d_pool, (size_t)3 * max_batch * poly_bytes));
    LR_HIP(hipMalloc((void **)&h->d_zero, poly_bytes));
    LR_HIP(hipMemsetAsync(h->d_zero, 0, poly_bytes, cQ->stream));
    LR_HIP(hipStreamSynchronize(cQ->stream));          // the contexts may be given another stream before the first call
    *out = h.release();
    return LR_OK;
    });
}

extern "C" int lr_collective_destroy(lr_collective *h) {
    return guarded([&]() -> int { return destroy_handle(h); });
}

typedef const unsigned char *bytes_t;

extern "C" int lr_collective_ckks_cks_share(lr_collective *h, int level, const lr_poly *sk_in, const lr_poly *sk_out, const lr_poly *c1,
                                            const uint8_t *e, int batch, lr_poly *share_out) {
    return guarded([&]() -> int { return ckks_cks_share(h, level, sk_in, sk_out, c1, e, batch, share_out, false); });
}
extern "C" int lr_collective_ckks_cks_share_device(lr_collective *h, int level, const lr_poly *sk_in, const lr_poly *sk_out, const lr_poly *c1,
                                                   const void *e, int batch, lr_poly *share_out) {
    return guarded([&]() -> int { return ckks_cks_share(h, level, sk_in, sk_out, c1, (bytes_t)e, batch, share_out, true); });
}
extern "C" int lr_collective_bfv_cks_share(lr_collective *h, const lr_poly *sk_in, const lr_poly *sk_out, const lr_poly *c1, const uint8_t *e,
                                           int batch, lr_poly *share_out) {
    return guarded([&]() -> int { return bfv_cks_share(h, sk_in, sk_out, c1, e, batch, share_out, false); });
}
extern "C" int lr_collective_bfv_cks_share_device(lr_collective *h, const lr_poly *sk_in, const lr_poly *sk_out, const lr_poly *c1, const void *e,
                                                  int batch, lr_poly *share_out) {
    return guarded([&]() -> int { return bfv_cks_share(h, sk_in, sk_out, c1, (bytes_t)e, batch, share_out, true); });
}
extern "C" int lr_collective_ckks_pcks_share(lr_collective *h, int level, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1,
                                             const lr_poly *c1, const uint8_t *u_coeff_bits, const uint8_t *u_sign_bits, const uint8_t *e0,
                                             const uint8_t *e1, int batch, lr_poly *out0, lr_poly *out1) {
    return guarded([&]() -> int {
        return ckks_pcks_share(h, level, sk, pk0, pk1, c1, PkRandom{u_coeff_bits, u_sign_bits, e0, e1}, batch, out0, out1, false);
    });
}
extern "C" int lr_collective_ckks_pcks_share_device(lr_collective *h, int level, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1,
                                                    const lr_poly *c1, const void *u_coeff_bits, const void *u_sign_bits, const void *e0,
                                                    const void *e1, int batch, lr_poly *out0, lr_poly *out1) {
    return guarded([&]() -> int {
        return ckks_pcks_share(h, level, sk, pk0, pk1, c1, PkRandom{(bytes_t)u_coeff_bits, (bytes_t)u_sign_bits, (bytes_t)e0, (bytes_t)e1}, batch,
                               out0, out1, true);
    });
}
extern "C" int lr_collective_bfv_pcks_share(lr_collective *h, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1, const lr_poly *c1,
                                            const uint8_t *u_coeff_bits, const uint8_t *u_sign_bits, const uint8_t *e0, const uint8_t *e1,
                                            int batch, lr_poly *out0, lr_poly *out1) {
    return guarded([&]() -> int {
        return bfv_pcks_share(h, sk, pk0, pk1, c1, PkRandom{u_coeff_bits, u_sign_bits, e0, e1}, batch, out0, out1, false);
    });
}
extern "C" int lr_collective_bfv_pcks_share_device(lr_collective *h, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1, const lr_poly *c1,
                                                   const void *u_coeff_bits, const void *u_sign_bits, const void *e0, const void *e1, int batch,
                                                   lr_poly *out0, lr_poly *out1) {
    return guarded([&]() -> int {
        return bfv_pcks_share(h, sk, pk0, pk1, c1, PkRandom{(bytes_t)u_coeff_bits, (bytes_t)u_sign_bits, (bytes_t)e0, (bytes_t)e1}, batch, out0,
                              out1, true);
    });
}
extern "C" int lr_collective_aggregate(lr_collective *h, int level, const lr_poly *base, const lr_poly *const *shares, int n_shares, lr_poly *out) {
    return guarded([&]() -> int { return fold_shares(h, h ? h->d_pool : nullptr, level, base, shares, n_shares, out); });
}
