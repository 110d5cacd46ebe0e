// lr_ckks_encryptor.cpp -- C ABI: lr_ckks_encryptor, pkEncryptor.encrypt and skEncryptor.encrypt (ckks/encryptor.go:179-237, 318-362) for a
// batch of ciphertexts on the device.  The randomness arrives in the compact form the reference's samplers decide before they write limbs
// (the format of lr_bfv_encryptor) and is expanded by the kernels of lr_ckks_encrypt.hip and lr_bfv_encrypt.hip.
// The host sanitizer build (tests/host_stub_build.py) compiles this unit with every other; the launchers of lr_ckks_encrypt.hip have their
// stand-in in tests/cpp/hipstub/stub_ckks_encrypt.cpp.  What it shares with lr_bfv_encryptor.cpp, lr_keygen.cpp and lr_collective.cpp is
// lr_qp_handle.hpp.
#include "lr_qp_handle.hpp"

// what newEncryptor builds (ckks/encryptor.go:100-119); the contexts, the scalars and the staging of the host-randomness entry points
// (max_batch * (N / 4 + 2 N) bytes) are QpHandle's.  cP == nullptr: only the fast forms
struct lr_ckks_encryptor : lr_host::QpHandle {
    lr_bext *bext = nullptr;                  // NewFastBasisExtender(contextQ, contextP), owned
    u64 *d_pool = nullptr;                    // polypool: three polys over Q||P for max_batch ciphertexts
    ~lr_ckks_encryptor() {
        if (d_pool) (void)hipFree(d_pool);
        if (bext) lr_bext_destroy(bext);
    }
};

namespace lr_host {
namespace {

// everything a call shares: the form against the handle, the level, the outputs, the plaintext
int check_call(const lr_ckks_encryptor *e, int fast, int level, const lr_poly *pt, int batch, const lr_poly *o0, const lr_poly *o1) {
    if (!fast && !e->cP) return fail(LR_ERR_ARG, "CKKS encryptor: modulus P is empty -> use the fast form instead (ckks/encryptor.go:139-142)");
    if (o0 == o1 || o0->d == o1->d) return fail(LR_ERR_ARG, "CKKS encryptor: the two components of the ciphertext are the same poly");
    if (level < 0 || level + 1 > e->nQ) return fail(LR_ERR_SHAPE, "CKKS encryptor: level out of range");
    if (batch < 1) return fail(LR_ERR_SHAPE, "CKKS encryptor: batch must be at least 1");
    if (batch > e->max_batch) return fail(LR_ERR_SHAPE, "batch exceeds the encryptor's max_batch");
    LR_TRY(e->check_poly(pt, level + 1, batch, true, "the plaintext"));
    LR_TRY(e->check_poly(o0, level + 1, batch, false, "the ciphertext"));
    LR_TRY(e->check_poly(o1, level + 1, batch, false, "the ciphertext"));
    if (!fast) LR_TRY(same_stream(e->cQ, e->cP));
    return LR_OK;
}

// SampleTernaryMontgomery and / or KYSampler.Sample into the pool, `ternary` + `noises` parts of `batch` polys from P.p[first] on
int expand(lr_ckks_encryptor *e, const Pools &P, int first, int ternary, const unsigned char *u_coeff, const unsigned char *u_sign, int noises,
           const unsigned char *e0, const unsigned char *e1, int limbs, int batch) {
    return expand_qp(e, 0, limbs, ternary, u_coeff, u_sign, noises, e0, e1, P.p[first], P.stride, P.part, batch);
}

// the forward transform over limbs 0 .. limbs - 1 of `parts` pool polys that lie back to back: one launch where the batch allows it
int ntt_parts(lr_ckks_encryptor *e, const Pools &P, int first, int parts, int limbs, int batch) {
    if ((long long)parts * batch <= 65535) {
        Rows r{P.p[first], P.stride, 0, 1};
        return run_ntt(e->cQ, false, r, r, 0, 1, limbs, parts * batch);
    }
    for (int k = first; k < first + parts; ++k) {
        Rows r{P.p[k], P.stride, 0, 1};
        LR_TRY(run_ntt(e->cQ, false, r, r, 0, 1, limbs, batch));
    }
    return LR_OK;
}

// gaussianSampler.SampleAndAdd on `comps` pool polys over Q||P (ring/gaussianSampler.go:254-275)
int sample_and_add(lr_ckks_encryptor *e, const Pools &P, int comps, const unsigned char *const *eb, int batch) {
    if (e->call_by_call) {
        for (int k = 0; k < comps; ++k) {   // the sampler's residues as a poly, then Context.Add
            LR_TRY(noise_qp(e, 0, 1, &eb[k], &P.p[2], P.stride, e->rows(), batch));
            LR_TRY(ewise_qp(e, true, LR_ADD, batch, P.p[k], P.stride, P.p[2], P.stride, P.p[k], P.stride));
        }
        return LR_OK;
    }
    return noise_qp(e, 1, comps, eb, P.p, P.stride, e->rows(), batch);
}

// ModDownPQ(level, pool, ct) (ring/ring_basis_extension.go:248-275): the P part is read at rows level + 1 .. of the pool poly (:256), as
// lr_ckks_encrypt_pk does; then Context.NTT over limbs 0 .. level
int moddown_then_ntt(lr_ckks_encryptor *e, int level, u64 *pool, long long stride, int batch, lr_poly *out) {
    LR_TRY(moddown_pq_core(e->bext, level, pool, stride, Rows{pool, stride, level + 1, 1}, batch, out, false));
    Rows r = rows_of(out);
    return run_ntt(e->cQ, false, r, r, 0, 1, level + 1, batch);
}

int add_plaintext(lr_ckks_encryptor *e, int level, const lr_poly *pt, int batch, lr_poly *o0) {
    return run_ewise(e->cQ, LR_ADD, level + 1, batch, o0->d, o0->stride(), pt->d, key_stride(pt, batch), o0->d, o0->stride(), nullptr);
}

// pkEncryptor.encrypt (ckks/encryptor.go:179-237) after the sampling
int encrypt_pk_on_device(lr_ckks_encryptor *e, bool fast, int level, const lr_poly *pk0, const lr_poly *pk1, const PkRandom &R,
                         const lr_poly *pt, int batch, lr_poly *o0, lr_poly *o1) {
    lr_context *cQ = e->cQ;
    const int n = (int)cQ->h.N, L1 = level + 1;
    const Pools P = pools_of(e, e->d_pool, batch);
    const lr_poly *pk[2] = {pk0, pk1};
    lr_poly *outs[2] = {o0, o1};
    const unsigned char *eb[2] = {R.e0, R.e1};
    if (fast && e->call_by_call) {
        LR_TRY(expand(e, P, 2, 1, R.u_coeff, R.u_sign, 0, nullptr, nullptr, L1, batch));                       // :187
        LR_TRY(ntt_parts(e, P, 2, 1, L1, batch));
        for (int k = 0; k < 2; ++k)                                                                           // :190-192
            LR_TRY(run_ewise(cQ, LR_MUL_MONT, L1, batch, P.p[2], P.stride, pk[k]->d, key_stride(pk[k], batch), outs[k]->d, outs[k]->stride(), nullptr));
        for (int k = 0; k < 2; ++k) {                                                                         // :195-200
            LR_TRY(expand(e, P, 0, 0, nullptr, nullptr, 1, eb[k], nullptr, L1, batch));
            LR_TRY(ntt_parts(e, P, 0, 1, L1, batch));
            LR_TRY(run_ewise(cQ, LR_ADD, L1, batch, outs[k]->d, outs[k]->stride(), P.p[0], P.stride, outs[k]->d, outs[k]->stride(), nullptr));
        }
        return add_plaintext(e, level, pt, batch, o0);                                                        // :234
    }
    if (fast) {     // u, e0, e1 expanded side by side, one transform over all three, one pass for both components
        LR_TRY(expand(e, P, 0, 1, R.u_coeff, R.u_sign, 2, R.e0, R.e1, L1, batch));
        LR_TRY(ntt_parts(e, P, 0, 3, L1, batch));
        CkksPkFastLaunch F;
        F.u = P.p[0]; F.e0 = P.p[1]; F.e1 = P.p[2];
        F.r_stride = P.stride;
        F.pk0 = pk0->d; F.pk0_stride = key_stride(pk0, batch);
        F.pk1 = pk1->d; F.pk1_stride = key_stride(pk1, batch);
        F.pt = pt->d; F.pt_stride = key_stride(pt, batch);
        F.out0 = o0->d; F.out0_stride = o0->stride();
        F.out1 = o1->d; F.out1_stride = o1->stride();
        F.n = n;
        F.lp = e->d_lp;
        LR_HIP(launch_ckks_pk_fast(F, L1, batch, cQ->stream));
        return LR_OK;
    }
    // through the special primes (:204-230): the launch sequence of lr_ckks_encrypt_pk, with u and the noise from the samplers' bytes
    const int rows = e->rows();
    LR_TRY(ternary_qp(e, P, R.u_coeff, R.u_sign, rows, batch));                                               // :206 SampleTernaryMontgomeryNTT(polypool[2], 0.5) over Q||P
    LR_TRY(ntt_qp(e, true, false, e->nQ, batch, P.p[2], P.stride, P.p[2], P.stride));
    if (e->call_by_call) {
        for (int k = 0; k < 2; ++k)      // :209-211
            LR_TRY(ewise_qp(e, true, LR_MUL_MONT, batch, P.p[2], P.stride, pk[k]->d, key_stride(pk[k], batch), P.p[k], P.stride));
        for (int k = 0; k < 2; ++k)      // :214-215
            LR_TRY(ntt_qp(e, true, true, e->nQ, batch, P.p[k], P.stride, P.p[k], P.stride));
    } else {
        LR_TRY(mul2_qp(e, P, pk0, pk1, rows, batch));
        if (2LL * batch <= 65535) LR_TRY(ntt_qp(e, true, true, e->nQ, 2 * batch, P.p[0], P.stride, P.p[0], P.stride));    // the two pools are back to back
        else for (int k = 0; k < 2; ++k) LR_TRY(ntt_qp(e, true, true, e->nQ, batch, P.p[k], P.stride, P.p[k], P.stride));
    }
    LR_TRY(sample_and_add(e, P, 2, eb, batch));                                                               // :218-220
    for (int k = 0; k < 2; ++k) LR_TRY(moddown_then_ntt(e, level, P.p[k], P.stride, batch, outs[k]));         // :223-230
    return add_plaintext(e, level, pt, batch, o0);                                                            // :234
}

// skEncryptor.encrypt (ckks/encryptor.go:318-362) after the sampling; crp is read only: the reference's ModDownNTTPQ transforms the P rows
// of its operand in place (ring_basis_extension.go:172-174), here those rows go through the pool
int encrypt_sk_on_device(lr_ckks_encryptor *e, bool fast, int level, const lr_poly *sk, const lr_poly *crp, const unsigned char *eb,
                         const lr_poly *pt, int batch, lr_poly *o0, lr_poly *o1) {
    lr_context *cQ = e->cQ;
    const int n = (int)cQ->h.N, L1 = level + 1;
    const Pools P = pools_of(e, e->d_pool, batch);
    const long long ss = key_stride(sk, batch);
    if (fast) {
        LR_TRY(expand(e, P, 0, 0, nullptr, nullptr, 1, eb, nullptr, L1, batch));                              // :327 SampleNTT(polypool[0])
        LR_TRY(ntt_parts(e, P, 0, 1, L1, batch));
        if (e->call_by_call) {
            LR_TRY(run_ewise(cQ, LR_MUL_MONT, L1, batch, crp->d, crp->stride(), sk->d, ss, o0->d, o0->stride(), nullptr));      // :324
            LR_TRY(run_ewise(cQ, LR_NEG, L1, batch, o0->d, o0->stride(), nullptr, 0, o0->d, o0->stride(), nullptr));            // :325
            LR_TRY(run_ewise(cQ, LR_ADD, L1, batch, o0->d, o0->stride(), P.p[0], P.stride, o0->d, o0->stride(), nullptr));      // :328
            LR_TRY(run_ewise(cQ, LR_COPY, L1, batch, crp->d, crp->stride(), nullptr, 0, o1->d, o1->stride(), nullptr));         // :330
            return add_plaintext(e, level, pt, batch, o0);                                                                      // :359
        }
        CkksSkFastLaunch F;
        F.crp = crp->d; F.crp_stride = crp->stride();
        F.sk = sk->d; F.sk_stride = ss;
        F.e = P.p[0]; F.e_stride = P.stride;
        F.pt = pt->d; F.pt_stride = key_stride(pt, batch);
        F.out0 = o0->d; F.out0_stride = o0->stride();
        F.out1 = o1->d; F.out1_stride = o1->stride();
        F.n = n;
        F.lp = e->d_lp;
        LR_HIP(launch_ckks_sk_fast(F, L1, batch, cQ->stream));
        return LR_OK;
    }
    if (e->call_by_call) {
        LR_TRY(ewise_qp(e, true, LR_MUL_MONT, batch, crp->d, crp->stride(), sk->d, ss, P.p[0], P.stride));    // :337
        LR_TRY(ewise_qp(e, true, LR_NEG, batch, P.p[0], P.stride, nullptr, 0, P.p[0], P.stride));             // :338
    } else {
        NegMulLaunch M;
        M.a = crp->d; M.a_stride = crp->stride();
        M.b = sk->d; M.b_stride = ss;
        M.out = P.p[0]; M.out_stride = P.stride;
        M.n = n;
        M.lp = e->d_lp;
        LR_HIP(launch_bfv_negmul(M, e->rows(), batch, cQ->stream));
    }
    LR_TRY(ntt_qp(e, true, true, e->nQ, batch, P.p[0], P.stride, P.p[0], P.stride));                          // :341
    LR_TRY(sample_and_add(e, P, 1, &eb, batch));                                                              // :344
    LR_TRY(moddown_pq_core(e->bext, level, P.p[0], P.stride, Rows{P.p[0], P.stride, level + 1, 1}, batch, o0, false));          // :348
    // :352 ModDownNTTPQ(level, crp, ct1): InvNTT of the P rows (rows |Q| .. of crp), extension, NTT, subtract-multiply against crp's Q rows
    Rows pP{P.p[1], P.stride, e->nQ, 1};
    if (e->call_by_call) {
        LR_TRY(ewise_qp(e, true, LR_COPY, batch, crp->d, crp->stride(), nullptr, 0, P.p[1], P.stride));
        LR_TRY(run_ntt(e->cP, true, pP, pP, 0, 1, e->nP, batch));
        LR_TRY(moddown_pq_core(e->bext, level, P.p[1], P.stride, pP, batch, o1, true));
    } else {        // the P rows are transformed out of crp into the pool, the Q rows are read where they are
        LR_TRY(run_ntt(e->cP, true, Rows{crp->d, crp->stride(), e->nQ, 1}, pP, 0, 1, e->nP, batch));
        LR_TRY(moddown_pq_core(e->bext, level, crp->d, crp->stride(), pP, batch, o1, true));
    }
    Rows r = rows_of(o0);
    LR_TRY(run_ntt(cQ, false, r, r, 0, 1, L1, batch));                                                        // :355
    return add_plaintext(e, level, pt, batch, o0);                                                            // :359
}

int encrypt_pk(lr_ckks_encryptor *e, int fast, int level, const lr_poly *pk0, const lr_poly *pk1, const unsigned char *u_coeff,
               const unsigned char *u_sign, const unsigned char *e0, const unsigned char *e1, const lr_poly *pt, int batch, lr_poly *o0,
               lr_poly *o1, bool on_device) {
    if (!e || !pk0 || !pk1 || !u_coeff || !u_sign || !e0 || !e1 || !pt || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_call(e, fast, level, pt, batch, o0, o1));
    const int key_limbs = fast ? e->nQ : e->nQ + e->nP;
    LR_TRY(e->check_poly(pk0, key_limbs, batch, true, "the public key"));
    LR_TRY(e->check_poly(pk1, key_limbs, batch, true, "the public key"));
    LR_HIP(hipSetDevice(e->device));
    PkRandom R{u_coeff, u_sign, e0, e1};
    if (!on_device) LR_TRY(e->stage_random(&R, batch));
    return encrypt_pk_on_device(e, fast != 0, level, pk0, pk1, R, pt, batch, o0, o1);
}

int encrypt_sk(lr_ckks_encryptor *e, int fast, int level, const lr_poly *sk, const lr_poly *crp, const unsigned char *eb, const lr_poly *pt,
               int batch, lr_poly *o0, lr_poly *o1, bool on_device) {
    if (!e || !sk || !crp || !eb || !pt || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_call(e, fast, level, pt, batch, o0, o1));
    const int key_limbs = fast ? e->nQ : e->nQ + e->nP;
    LR_TRY(e->check_poly(sk, key_limbs, batch, true, "the secret key"));
    LR_TRY(e->check_poly(crp, key_limbs, batch, false, "the uniform poly"));
    if (crp->d == o0->d || crp->d == o1->d) return fail(LR_ERR_ARG, "CKKS encryptor: the uniform poly is not modified and cannot be an output");
    LR_HIP(hipSetDevice(e->device));
    if (!on_device) LR_TRY(e->stage_random(&eb, (size_t)batch * (size_t)e->cQ->h.N));
    return encrypt_sk_on_device(e, fast != 0, level, sk, crp, eb, pt, batch, o0, o1);
}

}  // namespace
}  // namespace lr_host

extern "C" int lr_ckks_encryptor_create(lr_context *cQ, lr_context *cP, int max_batch, lr_ckks_encryptor **out) {
    return lr_ckks_encryptor_create_ex(cQ, cP, max_batch, nullptr, out);
}

extern "C" int lr_ckks_encryptor_create_ex(lr_context *cQ, lr_context *cP, int max_batch, const lr_options *options, lr_ckks_encryptor **out) {
    return guarded([&]() -> int {
    if (!cQ || !out) return fail(LR_ERR_ARG, "null argument");
    *out = nullptr;
    const char *name = "CKKS encryptor";
    Options parsed;
    LR_TRY(check_create(name, cQ, max_batch, options, &parsed));
    LR_TRY(check_pair(cQ, cP));
    std::unique_ptr<lr_ckks_encryptor> e(new lr_ckks_encryptor());
    LR_TRY(e->init(name, cQ, cP, max_batch, parsed));
    LR_HIP(hipSetDevice(cQ->device));
    if (cP) LR_TRY(lr_bext_create(cQ, cP, &e->bext));
    const size_t N = (size_t)cQ->h.N;
    LR_TRY(e->allocate((size_t)max_batch * (N / 4 + 2 * N)));
    LR_HIP(hipMalloc((void **)&e->d_pool, (size_t)3 * max_batch * e->rows() * N * sizeof(u64)));
    *out = e.release();
    return LR_OK;
    });
}

extern "C" int lr_ckks_encryptor_destroy(lr_ckks_encryptor *e) {
    return guarded([&]() -> int { return destroy_handle(e); });
}

extern "C" int lr_ckks_encryptor_encrypt_pk(lr_ckks_encryptor *e, int fast, int level, const lr_poly *pk0, const lr_poly *pk1,
                                            const uint8_t *u_coeff_bits, const uint8_t *u_sign_bits, const uint8_t *e0, const uint8_t *e1,
                                            const lr_poly *pt, int batch, lr_poly *o0, lr_poly *o1) {
    return guarded([&]() -> int { return encrypt_pk(e, fast, level, pk0, pk1, u_coeff_bits, u_sign_bits, e0, e1, pt, batch, o0, o1, false); });
}

extern "C" int lr_ckks_encryptor_encrypt_pk_device(lr_ckks_encryptor *e, int fast, int level, const lr_poly *pk0, const lr_poly *pk1,
                                                   const void *u_coeff_bits, const void *u_sign_bits, const void *e0, const void *e1,
                                                   const lr_poly *pt, int batch, lr_poly *o0, lr_poly *o1) {
    return guarded([&]() -> int {
        return encrypt_pk(e, fast, level, pk0, pk1, (const unsigned char *)u_coeff_bits, (const unsigned char *)u_sign_bits,
                          (const unsigned char *)e0, (const unsigned char *)e1, pt, batch, o0, o1, true);
    });
}

extern "C" int lr_ckks_encryptor_encrypt_sk(lr_ckks_encryptor *e, int fast, int level, const lr_poly *sk, const lr_poly *crp, const uint8_t *eb,
                                            const lr_poly *pt, int batch, lr_poly *o0, lr_poly *o1) {
    return guarded([&]() -> int { return encrypt_sk(e, fast, level, sk, crp, eb, pt, batch, o0, o1, false); });
}

extern "C" int lr_ckks_encryptor_encrypt_sk_device(lr_ckks_encryptor *e, int fast, int level, const lr_poly *sk, const lr_poly *crp,
                                                   const void *eb, const lr_poly *pt, int batch, lr_poly *o0, lr_poly *o1) {
    return guarded([&]() -> int { return encrypt_sk(e, fast, level, sk, crp, (const unsigned char *)eb, pt, batch, o0, o1, true); });
}
