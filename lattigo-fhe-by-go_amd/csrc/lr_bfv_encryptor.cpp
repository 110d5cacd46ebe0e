// lr_bfv_encryptor.cpp -- C ABI: lr_bfv_encryptor and lr_bfv_decryptor, pkEncryptor.encrypt / skEncryptor.encrypt (bfv/encryptor.go:169-223,
// 306-345) and decryptor.Decrypt (bfv/decryptor.go:55-75) for a batch of ciphertexts on the device.  The randomness arrives in the compact
// form the reference's samplers decide before they write limbs and is expanded by the kernels of lr_bfv_encrypt.hip.
// The host sanitizer build (tests/host_stub_build.py) compiles this unit with every other; the launchers of lr_bfv_encrypt.hip have their
// stand-in in tests/cpp/hipstub/stub_bfv_encrypt.cpp.  What it shares with lr_ckks_encryptor.cpp, lr_keygen.cpp and lr_collective.cpp is
// lr_qp_handle.hpp.
#include "lr_qp_handle.hpp"

// what newEncryptor builds (bfv/encryptor.go:100-119); the contexts, the scalars and the staging of the host-randomness entry points
// (max_batch * (N / 4 + 2 N) bytes) are QpHandle's.  cP == nullptr: only the fast forms
struct lr_bfv_encryptor : lr_host::QpHandle {
    lr_bext *bext = nullptr;                  // NewFastBasisExtender(contextQ, contextP), owned
    u64 *d_pool = nullptr;                    // polypool: three polys over Q||P for max_batch ciphertexts
    ~lr_bfv_encryptor() {
        if (d_pool) (void)hipFree(d_pool);
        if (bext) lr_bext_destroy(bext);
    }
};

// what bfv.NewDecryptor builds (bfv/decryptor.go:28-45): the pool, here one slot per ciphertext component
struct lr_bfv_decryptor {
    int device = 0;
    lr_context *cQ = nullptr;
    int max_batch = 0;
    bool call_by_call = false;
    Pool pool;
};

namespace lr_host {
namespace {

// everything a call shares: the form against the handle, the outputs, the plaintext
int check_call(const lr_bfv_encryptor *e, int fast, const lr_poly *pt, int batch, const lr_poly *o0, const lr_poly *o1) {
    if (!fast && !e->cP) return fail(LR_ERR_ARG, "BFV encryptor: modulus P is empty -> use the fast form instead (bfv/encryptor.go:123-125)");
    if (o0 == o1 || o0->d == o1->d) return fail(LR_ERR_ARG, "BFV encryptor: the two components of the ciphertext are the same poly");
    if (batch < 1) return fail(LR_ERR_SHAPE, "BFV encryptor: batch must be at least 1");
    if (batch > e->max_batch) return fail(LR_ERR_SHAPE, "batch exceeds the encryptor's max_batch");
    LR_TRY(e->check_poly(pt, e->nQ, batch, true, "the plaintext"));
    LR_TRY(e->check_poly(o0, e->nQ, batch, false, "the ciphertext"));
    LR_TRY(e->check_poly(o1, e->nQ, batch, false, "the ciphertext"));
    if (!fast) LR_TRY(same_stream(e->cQ, e->cP));
    return LR_OK;
}

// ModDownPQ(|Q| - 1, pool, ct) (ring/ring_basis_extension.go:249-275): the P part is rows |Q| .. of the pool poly
int moddown(lr_bfv_encryptor *e, u64 *pool, long long stride, int batch, lr_poly *out) {
    return moddown_pq_core(e->bext, e->nQ - 1, pool, stride, Rows{pool, stride, e->nQ, 1}, batch, out, false);
}

// pkEncryptor.encrypt (bfv/encryptor.go:169-223) after the sampling.  fast: :173-190 over Q; otherwise :194-216 over Q||P.  In the fast
// branch the reference leaves the two polys in its pool and never writes them to the ciphertext (v1.3.1); here they are the ciphertext.
int encrypt_pk_on_device(lr_bfv_encryptor *e, bool fast, const lr_poly *pk0, const lr_poly *pk1, const PkRandom &R, const lr_poly *pt, int batch,
                         lr_poly *o0, lr_poly *o1) {
    lr_context *cQ = e->cQ;
    const int rows = fast ? e->nQ : e->rows();
    const bool through_p = !fast;
    const Pools P = pools_of(e, e->d_pool, batch);
    const lr_poly *pk[2] = {pk0, pk1};
    lr_poly *outs[2] = {o0, o1};
    const unsigned char *eb[2] = {R.e0, R.e1};
    const long long ps = key_stride(pt, batch);
    LR_TRY(ternary_qp(e, P, R.u_coeff, R.u_sign, rows, batch));      // :176 / :196 SampleTernaryMontgomeryNTT(polypool[2], 0.5)
    LR_TRY(ntt_qp(e, through_p, false, e->nQ, batch, P.p[2], P.stride, P.p[2], P.stride));
    if (e->call_by_call) {
        for (int k = 0; k < 2; ++k)      // :178-179 / :200-201 MulCoeffsMontgomery(polypool[2], pk[k], polypool[k])
            LR_TRY(ewise_qp(e, through_p, LR_MUL_MONT, batch, P.p[2], P.stride, pk[k]->d, key_stride(pk[k], batch), P.p[k], P.stride));
        for (int k = 0; k < 2; ++k)      // :181-182 / :203-204 InvNTT
            LR_TRY(ntt_qp(e, through_p, true, e->nQ, batch, P.p[k], P.stride, P.p[k], P.stride));
        for (int k = 0; k < 2; ++k) {    // :185-190 / :207-212 gaussianSampler.Sample(polypool[2]); Add
            LR_TRY(noise_qp(e, 0, 1, &eb[k], &P.p[2], P.stride, rows, batch));
            LR_TRY(ewise_qp(e, through_p, LR_ADD, batch, P.p[k], P.stride, P.p[2], P.stride, P.p[k], P.stride));
        }
        if (fast) {
            LR_TRY(run_ewise(cQ, LR_ADD, e->nQ, batch, P.p[0], P.stride, pt->d, ps, o0->d, o0->stride(), nullptr));                   // :222
            return run_ewise(cQ, LR_COPY, e->nQ, batch, P.p[1], P.stride, nullptr, 0, o1->d, o1->stride(), nullptr);
        }
        for (int k = 0; k < 2; ++k) LR_TRY(moddown(e, P.p[k], P.stride, batch, outs[k]));                                            // :215-216
        return run_ewise(cQ, LR_ADD, e->nQ, batch, o0->d, o0->stride(), pt->d, ps, o0->d, o0->stride(), nullptr);                    // :222
    }
    LR_TRY(mul2_qp(e, P, pk0, pk1, rows, batch));
    LR_TRY(ntt_qp(e, through_p, true, e->nQ, 2 * batch, P.p[0], P.stride, P.p[0], P.stride));     // the two pools are back to back: one batch of 2 * batch
    // fast: the sums are the ciphertext, and the Add of the plaintext rides on component 0
    LR_TRY(noise_qp(e, 1, 2, eb, P.p, P.stride, rows, batch, fast ? outs : nullptr, fast ? pt : nullptr));
    if (fast) return LR_OK;
    for (int k = 0; k < 2; ++k) LR_TRY(moddown(e, P.p[k], P.stride, batch, outs[k]));
    return run_ewise(cQ, LR_ADD, e->nQ, batch, o0->d, o0->stride(), pt->d, ps, o0->d, o0->stride(), nullptr);
}

// skEncryptor.encrypt (bfv/encryptor.go:306-345) after the sampling; crp is read, the reference's in-place InvNTT of it (:331) works on
// its copy in polypool[1] (encryptFromCRP, :296-304)
int encrypt_sk_on_device(lr_bfv_encryptor *e, bool fast, const lr_poly *sk, const lr_poly *crp, const unsigned char *eb, const lr_poly *pt,
                         int batch, lr_poly *o0, lr_poly *o1) {
    lr_context *cQ = e->cQ;
    const int rows = fast ? e->nQ : e->rows();
    const bool through_p = !fast;
    const Pools P = pools_of(e, e->d_pool, batch);
    const long long ps = key_stride(pt, batch), ss = key_stride(sk, batch);
    u64 *crp_d = crp->d;
    // fast: the ciphertext's polys take the place of the pool (:314-320)
    u64 *acc = fast ? o0->d : P.p[0], *a_out = fast ? o1->d : P.p[1];
    const long long acc_s = fast ? o0->stride() : P.stride, a_s = fast ? o1->stride() : P.stride;
    if (e->call_by_call) {
        LR_TRY(ewise_qp(e, through_p, LR_MUL_MONT, batch, crp_d, crp->stride(), sk->d, ss, acc, acc_s));      // :314 / :326
        LR_TRY(ewise_qp(e, through_p, LR_NEG, batch, acc, acc_s, nullptr, 0, acc, acc_s));                    // :315 / :327
        LR_TRY(ntt_qp(e, through_p, true, e->nQ, batch, acc, acc_s, acc, acc_s));                             // :317 / :330
        if (fast) {
            LR_TRY(ntt_qp(e, false, true, e->nQ, batch, crp_d, crp->stride(), a_out, a_s));                   // :318
        } else {
            LR_TRY(ewise_qp(e, true, LR_COPY, batch, crp_d, crp->stride(), nullptr, 0, a_out, a_s));          // :300
            LR_TRY(ntt_qp(e, true, true, e->nQ, batch, a_out, a_s, a_out, a_s));                              // :331
        }
        LR_TRY(noise_qp(e, 0, 1, &eb, &P.p[2], P.stride, rows, batch));                                       // :320 / :333
        LR_TRY(ewise_qp(e, through_p, LR_ADD, batch, acc, acc_s, P.p[2], P.stride, acc, acc_s));
        if (!fast) {
            LR_TRY(moddown(e, P.p[0], P.stride, batch, o0));                                                  // :335-336
            LR_TRY(moddown(e, P.p[1], P.stride, batch, o1));
        }
        return run_ewise(cQ, LR_ADD, e->nQ, batch, o0->d, o0->stride(), pt->d, ps, o0->d, o0->stride(), nullptr);   // :344
    }
    NegMulLaunch M;
    M.a = crp_d; M.a_stride = crp->stride();
    M.b = sk->d; M.b_stride = ss;
    M.out = acc; M.out_stride = acc_s;
    M.n = (int)cQ->h.N;
    M.lp = e->d_lp;
    LR_HIP(launch_bfv_negmul(M, rows, batch, cQ->stream));
    LR_TRY(ntt_qp(e, through_p, true, e->nQ, batch, acc, acc_s, acc, acc_s));
    LR_TRY(ntt_qp(e, through_p, true, e->nQ, batch, crp_d, crp->stride(), a_out, a_s));
    LR_TRY(noise_qp(e, 1, 1, &eb, &acc, acc_s, rows, batch, nullptr, fast ? pt : nullptr));   // fast: the Add of the plaintext rides on the sampler's Add
    if (fast) return LR_OK;
    LR_TRY(moddown(e, P.p[0], P.stride, batch, o0));
    LR_TRY(moddown(e, P.p[1], P.stride, batch, o1));
    return run_ewise(cQ, LR_ADD, e->nQ, batch, o0->d, o0->stride(), pt->d, ps, o0->d, o0->stride(), nullptr);
}

int encrypt_pk(lr_bfv_encryptor *e, int fast, const lr_poly *pk0, const lr_poly *pk1, const unsigned char *u_coeff, const unsigned char *u_sign,
               const unsigned char *e0, const unsigned char *e1, const lr_poly *pt, int batch, lr_poly *o0, lr_poly *o1, bool on_device) {
    if (!e || !pk0 || !pk1 || !u_coeff || !u_sign || !e0 || !e1 || !pt || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_call(e, fast, pt, batch, o0, o1));
    const int key_limbs = fast ? e->nQ : e->nQ + e->nP;
    LR_TRY(e->check_poly(pk0, key_limbs, batch, true, "the public key"));
    LR_TRY(e->check_poly(pk1, key_limbs, batch, true, "the public key"));
    LR_HIP(hipSetDevice(e->device));
    PkRandom R{u_coeff, u_sign, e0, e1};
    if (!on_device) LR_TRY(e->stage_random(&R, batch));
    return encrypt_pk_on_device(e, fast != 0, pk0, pk1, R, pt, batch, o0, o1);
}

int encrypt_sk(lr_bfv_encryptor *e, int fast, const lr_poly *sk, const lr_poly *crp, const unsigned char *eb, const lr_poly *pt, int batch,
               lr_poly *o0, lr_poly *o1, bool on_device) {
    if (!e || !sk || !crp || !eb || !pt || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_call(e, fast, pt, batch, o0, o1));
    const int key_limbs = fast ? e->nQ : e->nQ + e->nP;
    LR_TRY(e->check_poly(sk, key_limbs, batch, true, "the secret key"));
    LR_TRY(e->check_poly(crp, key_limbs, batch, false, "the uniform poly"));
    if (crp->d == o0->d || crp->d == o1->d) return fail(LR_ERR_ARG, "BFV encryptor: the uniform poly is not modified and cannot be an output");
    LR_HIP(hipSetDevice(e->device));
    if (!on_device) LR_TRY(e->stage_random(&eb, (size_t)batch * (size_t)e->cQ->h.N));
    return encrypt_sk_on_device(e, fast != 0, sk, crp, eb, pt, batch, o0, o1);
}

// decryptor.Decrypt (bfv/decryptor.go:55-75)
int decrypt(lr_bfv_decryptor *d, const lr_poly *const *ct, int degree, const lr_poly *sk, lr_poly *pt, int batch) {
    if (!d || !ct || !sk || !pt) return fail(LR_ERR_ARG, "null argument");
    if (degree < 0) return fail(LR_ERR_ARG, "negative degree");
    for (int i = 0; i <= degree; ++i)
        if (!ct[i]) return fail(LR_ERR_ARG, "null argument");
    lr_context *cQ = d->cQ;
    const int nQ = cQ->h.L();
    if (batch < 1) return fail(LR_ERR_SHAPE, "BFV decryptor: batch must be at least 1");
    if (batch > d->max_batch) return fail(LR_ERR_SHAPE, "batch exceeds the decryptor's max_batch");
    auto check = [&](const lr_poly *p, bool broadcast, const char *what) -> int {
        if (p->ctx != cQ) return fail(LR_ERR_ARG, std::string("BFV decryptor: ") + what + " belongs to another context");
        if (p->N != cQ->h.N || p->limbs < nQ) return fail(LR_ERR_SHAPE, std::string("BFV decryptor: ") + what + " has too few limbs");
        if (p->batch != batch && !(broadcast && p->batch == 1)) return fail(LR_ERR_SHAPE, std::string("BFV decryptor: batch differs from the batch of ") + what);
        return LR_OK;
    };
    for (int i = 0; i <= degree; ++i) LR_TRY(check(ct[i], false, "the ciphertext"));
    LR_TRY(check(pt, false, "the plaintext"));
    LR_TRY(check(sk, true, "the secret key"));
    LR_HIP(hipSetDevice(d->device));
    const long long n = (long long)cQ->h.N, sQ = (long long)nQ * n, slot = (long long)batch * sQ, ss = key_stride(sk, batch);
    auto ntt_in = [&](int first, int count, u64 *dst) -> int {     // components first .. first + count - 1, back to back, as one batch
        return run_ntt(cQ, false, Rows{ct[first]->d, ct[first]->stride(), 0, 1}, Rows{dst, sQ, 0, 1}, 0, 1, nQ, count * batch);
    };
    if (d->call_by_call) {
        // the reference's call order: one transform per component, between the Horner steps; the accumulator and polypool are pool slots
        LR_TRY(d->pool.ensure(cQ, (size_t)(2 * slot)));
        u64 *acc = d->pool.d, *tmp = d->pool.d + slot;
        LR_TRY(ntt_in(degree, 1, acc));                                                                          // :58
        for (int i = degree; i > 0; --i) {
            LR_TRY(run_ewise(cQ, LR_MUL_MONT, nQ, batch, acc, sQ, sk->d, ss, acc, sQ, nullptr));                  // :61
            LR_TRY(ntt_in(i - 1, 1, tmp));                                                                       // :62
            LR_TRY(run_ewise(cQ, LR_ADD, nQ, batch, acc, sQ, tmp, sQ, acc, sQ, nullptr));                         // :63
            if ((i & 7) == 7) LR_TRY(run_ewise(cQ, LR_REDUCE, nQ, batch, acc, sQ, nullptr, 0, acc, sQ, nullptr)); // :66
        }
        if ((degree & 7) != 7) LR_TRY(run_ewise(cQ, LR_REDUCE, nQ, batch, acc, sQ, nullptr, 0, acc, sQ, nullptr));// :71
        return run_ntt(cQ, true, Rows{acc, sQ, 0, 1}, rows_of(pt), 0, 1, nQ, batch);                             // :74
    }
    // every component transformed into its pool slot: components that lie back to back in memory share a launch
    LR_TRY(d->pool.ensure(cQ, (size_t)((degree + 1) * slot)));
    for (int i = 0, j; i <= degree; i = j) {
        j = i + 1;
        while (j <= degree && ct[j]->stride() == ct[i]->stride() && ct[j]->d == ct[j - 1]->d + (long long)batch * ct[i]->stride() &&
               (long long)(j - i + 1) * batch <= 65535)
            ++j;
        LR_TRY(ntt_in(i, j - i, d->pool.d + i * slot));
    }
    if (degree <= kHornerMaxDegree) {
        HornerLaunch H;
        std::memset(&H, 0, sizeof H);
        for (int i = 0; i <= degree; ++i) {
            H.ct[i] = d->pool.d + i * slot;
            H.ct_stride[i] = sQ;
        }
        H.sk = sk->d;
        H.sk_stride = ss;
        H.out = pt->d;
        H.out_stride = pt->stride();
        H.degree = degree;
        H.n = (int)n;
        H.lp = cQ->d_lp;
        LR_HIP(launch_horner(H, nQ, batch, cQ->stream));
        Rows r = rows_of(pt);
        return run_ntt(cQ, true, r, r, 0, 1, nQ, batch);
    }
    u64 *acc = d->pool.d + degree * slot;
    for (int i = degree; i > 0; --i) {
        LR_TRY(run_ewise(cQ, LR_MUL_MONT, nQ, batch, acc, sQ, sk->d, ss, acc, sQ, nullptr));
        LR_TRY(run_ewise(cQ, LR_ADD, nQ, batch, acc, sQ, d->pool.d + (i - 1) * slot, sQ, acc, sQ, nullptr));
        if ((i & 7) == 7) LR_TRY(run_ewise(cQ, LR_REDUCE, nQ, batch, acc, sQ, nullptr, 0, acc, sQ, nullptr));
    }
    if ((degree & 7) != 7) LR_TRY(run_ewise(cQ, LR_REDUCE, nQ, batch, acc, sQ, nullptr, 0, acc, sQ, nullptr));
    return run_ntt(cQ, true, Rows{acc, sQ, 0, 1}, rows_of(pt), 0, 1, nQ, batch);
}

}  // namespace
}  // namespace lr_host

extern "C" int lr_bfv_encryptor_create(lr_context *cQ, lr_context *cP, int max_batch, lr_bfv_encryptor **out) {
    return lr_bfv_encryptor_create_ex(cQ, cP, max_batch, nullptr, out);
}

extern "C" int lr_bfv_encryptor_create_ex(lr_context *cQ, lr_context *cP, int max_batch, const lr_options *options, lr_bfv_encryptor **out) {
    return guarded([&]() -> int {
    if (!cQ || !out) return fail(LR_ERR_ARG, "null argument");
    *out = nullptr;
    const char *name = "BFV encryptor";
    Options parsed;
    LR_TRY(check_create(name, cQ, max_batch, options, &parsed));
    LR_TRY(check_pair(cQ, cP));
    std::unique_ptr<lr_bfv_encryptor> e(new lr_bfv_encryptor());
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

extern "C" int lr_bfv_encryptor_destroy(lr_bfv_encryptor *e) {
    return guarded([&]() -> int { return destroy_handle(e); });
}

extern "C" int lr_bfv_encrypt_pk(lr_bfv_encryptor *e, int fast, const lr_poly *pk0, const lr_poly *pk1, const uint8_t *u_coeff_bits,
                                 const uint8_t *u_sign_bits, const uint8_t *e0, const uint8_t *e1, const lr_poly *pt, int batch, lr_poly *o0,
                                 lr_poly *o1) {
    return guarded([&]() -> int { return encrypt_pk(e, fast, pk0, pk1, u_coeff_bits, u_sign_bits, e0, e1, pt, batch, o0, o1, false); });
}

extern "C" int lr_bfv_encrypt_pk_device(lr_bfv_encryptor *e, int fast, const lr_poly *pk0, const lr_poly *pk1, const void *u_coeff_bits,
                                        const void *u_sign_bits, const void *e0, const void *e1, const lr_poly *pt, int batch, lr_poly *o0,
                                        lr_poly *o1) {
    return guarded([&]() -> int {
        return encrypt_pk(e, fast, pk0, pk1, (const unsigned char *)u_coeff_bits, (const unsigned char *)u_sign_bits, (const unsigned char *)e0,
                          (const unsigned char *)e1, pt, batch, o0, o1, true);
    });
}

extern "C" int lr_bfv_encrypt_sk(lr_bfv_encryptor *e, int fast, const lr_poly *sk, const lr_poly *crp, const uint8_t *eb, const lr_poly *pt,
                                 int batch, lr_poly *o0, lr_poly *o1) {
    return guarded([&]() -> int { return encrypt_sk(e, fast, sk, crp, eb, pt, batch, o0, o1, false); });
}

extern "C" int lr_bfv_encrypt_sk_device(lr_bfv_encryptor *e, int fast, const lr_poly *sk, const lr_poly *crp, const void *eb, const lr_poly *pt,
                                        int batch, lr_poly *o0, lr_poly *o1) {
    return guarded([&]() -> int { return encrypt_sk(e, fast, sk, crp, (const unsigned char *)eb, pt, batch, o0, o1, true); });
}

extern "C" int lr_bfv_decryptor_create(lr_context *cQ, int max_batch, lr_bfv_decryptor **out) {
    return guarded([&]() -> int {
    if (!cQ || !out) return fail(LR_ERR_ARG, "null argument");
    *out = nullptr;
    if (max_batch < 1 || max_batch > 65535) return fail(LR_ERR_ARG, "max_batch must be in 1 .. 65535");
    Options parsed = cQ->opt;
    parsed.apply_env();
    std::unique_ptr<lr_bfv_decryptor> d(new lr_bfv_decryptor());
    d->cQ = cQ;
    d->device = cQ->device;
    d->max_batch = max_batch;
    d->call_by_call = parsed.no_epilogue;
    *out = d.release();
    return LR_OK;
    });
}

extern "C" int lr_bfv_decryptor_destroy(lr_bfv_decryptor *d) {
    return guarded([&]() -> int {
    if (!d) return LR_OK;
    (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();
    delete d;
    return LR_OK;
    });
}

extern "C" int lr_bfv_decrypt(lr_bfv_decryptor *d, const lr_poly *const *ct, int degree, const lr_poly *sk, lr_poly *pt_out, int batch) {
    return guarded([&]() -> int { return decrypt(d, ct, degree, sk, pt_out, batch); });
}
