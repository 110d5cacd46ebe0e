// lr_ckks_encryptor.cpp -- C ABI: lr_ckks_encryptor, pkEncryptor.encrypt and skEncryptor.encrypt (ckks/encryptor.go:179-237, 318-362) for a
// batch of ciphertexts on the device.  The randomness arrives in the compact form the reference's samplers decide before they write limbs
// (the format of lr_bfv_encryptor) and is expanded by the kernels of lr_ckks_encrypt.hip and lr_bfv_encrypt.hip.
// The unit's name keeps it out of the lr_abi_*.cpp set that the shared sanitizer build links against its fixed launch stubs: the launchers
// it calls have a stand-in of their own (tests/cpp/ckks_encryptor_stub.cpp).  The small helpers it shares with lr_bfv_encryptor.cpp are
// copies: that unit stays as it is.
#include "lr_host.hpp"

// what newEncryptor builds (ckks/encryptor.go:100-119), plus the staging of the host-randomness entry points
struct lr_ckks_encryptor {
    int device = 0;
    lr_context *cQ = nullptr, *cP = nullptr;  // cP == nullptr: "modulus P is empty", only the fast forms
    lr_bext *bext = nullptr;                  // NewFastBasisExtender(contextQ, contextP), owned
    int nQ = 0, nP = 0, max_batch = 0;
    bool call_by_call = false;                // Options::no_epilogue: the reference's call-by-call shape
    LimbScalars one, minus_one;               // matrixTernaryMontgomery rows 1 and 2 (ring/ring_context.go:119-122) per limb of Q||P
    LimbParams *d_lp = nullptr;               // the limb constants of contextQP: contextQ's, then contextP's
    u64 *d_pool = nullptr;                    // polypool: three polys over Q||P for max_batch ciphertexts
    unsigned char *d_rand = nullptr;          // the host-randomness entry points' bytes on the device ...
    unsigned char *h_rand = nullptr;          // ... and pinned: max_batch * (N / 4 + 2 N)
    hipEvent_t staged = nullptr;              // the last copy out of h_rand: the next call waits for it before it refills the buffer
    ~lr_ckks_encryptor() {
        for (void *p : {(void *)d_lp, (void *)d_pool, (void *)d_rand})
            if (p) (void)hipFree(p);
        if (h_rand) (void)hipHostFree(h_rand);
        if (staged) (void)hipEventDestroy(staged);
        if (bext) lr_bext_destroy(bext);
    }
};

namespace lr_host {
namespace {

struct PkRandom { const unsigned char *u_coeff, *u_sign, *e0, *e1; };

long long key_stride(const lr_poly *p, int batch) { return p->batch == 1 && batch > 1 ? 0 : p->stride(); }

// a poly of the handle's contextQ with at least `limbs` limbs and the call's batch (or, where allowed, one poly for the whole batch)
int check_poly(const lr_ckks_encryptor *e, const lr_poly *p, int limbs, int batch, bool broadcast, const char *what) {
    if (p->ctx != e->cQ) return fail(LR_ERR_ARG, std::string("CKKS encryptor: ") + what + " belongs to another context");
    if (p->N != e->cQ->h.N || p->limbs < limbs) return fail(LR_ERR_SHAPE, std::string("CKKS encryptor: ") + what + " has too few limbs");
    if (p->batch != batch && !(broadcast && p->batch == 1)) return fail(LR_ERR_SHAPE, std::string("CKKS encryptor: batch differs from the batch of ") + what);
    return LR_OK;
}

// everything a call shares: the form against the handle, the level, the outputs, the plaintext
int check_call(const lr_ckks_encryptor *e, int fast, int level, const lr_poly *pt, int batch, const lr_poly *o0, const lr_poly *o1) {
    if (!fast && !e->cP) return fail(LR_ERR_ARG, "CKKS encryptor: modulus P is empty -> use the fast form instead (ckks/encryptor.go:139-142)");
    if (o0 == o1 || o0->d == o1->d) return fail(LR_ERR_ARG, "CKKS encryptor: the two components of the ciphertext are the same poly");
    if (level < 0 || level + 1 > e->nQ) return fail(LR_ERR_SHAPE, "CKKS encryptor: level out of range");
    if (batch < 1) return fail(LR_ERR_SHAPE, "CKKS encryptor: batch must be at least 1");
    if (batch > e->max_batch) return fail(LR_ERR_SHAPE, "batch exceeds the encryptor's max_batch");
    LR_TRY(check_poly(e, pt, level + 1, batch, true, "the plaintext"));
    LR_TRY(check_poly(e, o0, level + 1, batch, false, "the ciphertext"));
    LR_TRY(check_poly(e, o1, level + 1, batch, false, "the ciphertext"));
    if (!fast) LR_TRY(same_stream(e->cQ, e->cP));
    return LR_OK;
}

// the three pool polys of a call, back to back: [3][batch][|Q| + |P|][N]
struct Pools {
    u64 *p[3];
    long long stride, part;
};
Pools pools_of(const lr_ckks_encryptor *e, int batch) {
    const long long n = (long long)e->cQ->h.N, s = (long long)(e->nQ + e->nP) * n;
    return Pools{{e->d_pool, e->d_pool + batch * s, e->d_pool + 2 * batch * s}, s, batch * s};
}

// one Context call of contextQP on rows inside the pools: the Q rows under contextQ, the P rows under contextP
int ewise_qp(lr_ckks_encryptor *e, int op, int batch, const u64 *a, long long a_stride, const u64 *b, long long b_stride, u64 *out,
             long long out_stride) {
    const long long offP = (long long)e->nQ * (long long)e->cQ->h.N;
    LR_TRY(run_ewise(e->cQ, op, e->nQ, batch, a, a_stride, b, b_stride, out, out_stride, nullptr));
    return run_ewise(e->cP, op, e->nP, batch, a + offP, a_stride, b ? b + offP : nullptr, b_stride, out + offP, out_stride, nullptr);
}

int ntt_qp(lr_ckks_encryptor *e, bool inverse, int batch, u64 *in, long long in_stride, u64 *out, long long out_stride) {
    LR_TRY(run_ntt(e->cQ, inverse, Rows{in, in_stride, 0, 1}, Rows{out, out_stride, 0, 1}, 0, 1, e->nQ, batch));
    return run_ntt(e->cP, inverse, Rows{in, in_stride, e->nQ, 1}, Rows{out, out_stride, e->nQ, 1}, 0, 1, e->nP, batch);
}

// SampleTernaryMontgomery and / or KYSampler.Sample into the pool, `ternary` + `noises` parts of `batch` polys from P.p[first] on
int expand(lr_ckks_encryptor *e, const Pools &P, int first, int ternary, const unsigned char *u_coeff, const unsigned char *u_sign, int noises,
           const unsigned char *e0, const unsigned char *e1, int limbs, int batch) {
    CkksExpandLaunch X;
    std::memset(&X, 0, sizeof X);
    X.coeff_bits = u_coeff;
    X.sign_bits = u_sign;
    X.e[0] = e0;
    X.e[1] = e1;
    X.out = P.p[first];
    X.out_stride = P.stride;
    X.part_stride = P.part;
    X.n = (int)e->cQ->h.N;
    X.ternary = ternary;
    X.noises = noises;
    X.one = e->one;
    X.minus_one = e->minus_one;
    X.lp = e->d_lp;
    LR_HIP(launch_ckks_expand(X, limbs, batch, e->cQ->stream));
    return LR_OK;
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
    const int rows = e->nQ + e->nP;
    if (e->call_by_call) {
        for (int k = 0; k < comps; ++k) {   // the sampler's residues as a poly, then Context.Add
            NoiseLaunch L;
            std::memset(&L, 0, sizeof L);
            L.out[0] = P.p[2];
            L.out_stride[0] = P.stride;
            L.e[0] = eb[k];
            L.n = (int)e->cQ->h.N;
            L.lp = e->d_lp;
            LR_HIP(launch_bfv_noise(L, 1, rows, batch, e->cQ->stream));
            LR_TRY(ewise_qp(e, LR_ADD, batch, P.p[k], P.stride, P.p[2], P.stride, P.p[k], P.stride));
        }
        return LR_OK;
    }
    NoiseLaunch L;
    std::memset(&L, 0, sizeof L);
    for (int k = 0; k < comps; ++k) {
        L.x[k] = L.out[k] = P.p[k];
        L.x_stride[k] = L.out_stride[k] = P.stride;
        L.e[k] = eb[k];
    }
    L.n = (int)e->cQ->h.N;
    L.add = 1;
    L.lp = e->d_lp;
    LR_HIP(launch_bfv_noise(L, comps, rows, batch, e->cQ->stream));
    return LR_OK;
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
    const Pools P = pools_of(e, batch);
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
    const int rows = e->nQ + e->nP;
    {   // :206 SampleTernaryMontgomeryNTT(polypool[2], 0.5) over Q||P
        TernaryLaunch T;
        T.coeff_bits = R.u_coeff;
        T.sign_bits = R.u_sign;
        T.out = P.p[2];
        T.out_stride = P.stride;
        T.n = n;
        T.one = e->one;
        T.minus_one = e->minus_one;
        LR_HIP(launch_bfv_ternary(T, rows, batch, cQ->stream));
        LR_TRY(ntt_qp(e, false, batch, P.p[2], P.stride, P.p[2], P.stride));
    }
    if (e->call_by_call) {
        for (int k = 0; k < 2; ++k)      // :209-211
            LR_TRY(ewise_qp(e, LR_MUL_MONT, batch, P.p[2], P.stride, pk[k]->d, key_stride(pk[k], batch), P.p[k], P.stride));
        for (int k = 0; k < 2; ++k)      // :214-215
            LR_TRY(ntt_qp(e, true, batch, P.p[k], P.stride, P.p[k], P.stride));
    } else {
        Mul2Launch M;                    // both products in one pass over u, all rows of Q||P in one launch
        M.a = P.p[2]; M.a_stride = P.stride;
        M.b0 = pk0->d; M.b0_stride = key_stride(pk0, batch);
        M.b1 = pk1->d; M.b1_stride = key_stride(pk1, batch);
        M.out0 = P.p[0]; M.out1 = P.p[1];
        M.out0_stride = M.out1_stride = P.stride;
        M.n = n;
        M.lp = e->d_lp;
        LR_HIP(launch_mul2(M, rows, batch, cQ->stream));
        if (2LL * batch <= 65535) LR_TRY(ntt_qp(e, true, 2 * batch, P.p[0], P.stride, P.p[0], P.stride));    // the two pools are back to back
        else for (int k = 0; k < 2; ++k) LR_TRY(ntt_qp(e, true, batch, P.p[k], P.stride, P.p[k], P.stride));
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
    const Pools P = pools_of(e, batch);
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
    const int rows = e->nQ + e->nP;
    if (e->call_by_call) {
        LR_TRY(ewise_qp(e, LR_MUL_MONT, batch, crp->d, crp->stride(), sk->d, ss, P.p[0], P.stride));          // :337
        LR_TRY(ewise_qp(e, LR_NEG, batch, P.p[0], P.stride, nullptr, 0, P.p[0], P.stride));                   // :338
    } else {
        NegMulLaunch M;
        M.a = crp->d; M.a_stride = crp->stride();
        M.b = sk->d; M.b_stride = ss;
        M.out = P.p[0]; M.out_stride = P.stride;
        M.n = n;
        M.lp = e->d_lp;
        LR_HIP(launch_bfv_negmul(M, rows, batch, cQ->stream));
    }
    LR_TRY(ntt_qp(e, true, batch, P.p[0], P.stride, P.p[0], P.stride));                                       // :341
    LR_TRY(sample_and_add(e, P, 1, &eb, batch));                                                              // :344
    LR_TRY(moddown_pq_core(e->bext, level, P.p[0], P.stride, Rows{P.p[0], P.stride, level + 1, 1}, batch, o0, false));          // :348
    // :352 ModDownNTTPQ(level, crp, ct1): InvNTT of the P rows (rows |Q| .. of crp), extension, NTT, subtract-multiply against crp's Q rows
    Rows pP{P.p[1], P.stride, e->nQ, 1};
    if (e->call_by_call) {
        LR_TRY(ewise_qp(e, LR_COPY, batch, crp->d, crp->stride(), nullptr, 0, P.p[1], P.stride));
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

// the caller's bytes through the pinned buffer to the device, pieces one behind the other; the caller's arrays are free on return
int stage_random(lr_ckks_encryptor *e, const unsigned char *const *src, const size_t *bytes, int pieces, const unsigned char **dev) {
    LR_HIP(hipEventSynchronize(e->staged));               // the copy of the call before has left the pinned buffer
    size_t off = 0;
    for (int i = 0; i < pieces; ++i) {
        std::memcpy(e->h_rand + off, src[i], bytes[i]);
        dev[i] = e->d_rand + off;
        off += bytes[i];
    }
    LR_HIP(hipMemcpyAsync(e->d_rand, e->h_rand, off, hipMemcpyHostToDevice, e->cQ->stream));
    LR_HIP(hipEventRecord(e->staged, e->cQ->stream));
    return LR_OK;
}

int encrypt_pk(lr_ckks_encryptor *e, int fast, int level, const lr_poly *pk0, const lr_poly *pk1, const unsigned char *u_coeff,
               const unsigned char *u_sign, const unsigned char *e0, const unsigned char *e1, const lr_poly *pt, int batch, lr_poly *o0,
               lr_poly *o1, bool on_device) {
    if (!e || !pk0 || !pk1 || !u_coeff || !u_sign || !e0 || !e1 || !pt || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_call(e, fast, level, pt, batch, o0, o1));
    const int key_limbs = fast ? e->nQ : e->nQ + e->nP;
    LR_TRY(check_poly(e, pk0, key_limbs, batch, true, "the public key"));
    LR_TRY(check_poly(e, pk1, key_limbs, batch, true, "the public key"));
    LR_HIP(hipSetDevice(e->device));
    PkRandom R{u_coeff, u_sign, e0, e1};
    if (!on_device) {
        const size_t N = (size_t)e->cQ->h.N, plane = (size_t)batch * (N >> 3), noise = (size_t)batch * N;
        const unsigned char *src[4] = {u_coeff, u_sign, e0, e1}, *dev[4];
        const size_t bytes[4] = {plane, plane, noise, noise};
        LR_TRY(stage_random(e, src, bytes, 4, dev));
        R = PkRandom{dev[0], dev[1], dev[2], dev[3]};
    }
    return encrypt_pk_on_device(e, fast != 0, level, pk0, pk1, R, pt, batch, o0, o1);
}

int encrypt_sk(lr_ckks_encryptor *e, int fast, int level, const lr_poly *sk, const lr_poly *crp, const unsigned char *eb, const lr_poly *pt,
               int batch, lr_poly *o0, lr_poly *o1, bool on_device) {
    if (!e || !sk || !crp || !eb || !pt || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_call(e, fast, level, pt, batch, o0, o1));
    const int key_limbs = fast ? e->nQ : e->nQ + e->nP;
    LR_TRY(check_poly(e, sk, key_limbs, batch, true, "the secret key"));
    LR_TRY(check_poly(e, crp, key_limbs, batch, false, "the uniform poly"));
    if (crp->d == o0->d || crp->d == o1->d) return fail(LR_ERR_ARG, "CKKS encryptor: the uniform poly is not modified and cannot be an output");
    LR_HIP(hipSetDevice(e->device));
    if (!on_device) {
        const unsigned char *src[1] = {eb}, *dev[1];
        const size_t bytes[1] = {(size_t)batch * (size_t)e->cQ->h.N};
        LR_TRY(stage_random(e, src, bytes, 1, dev));
        eb = dev[0];
    }
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
    Options parsed = cQ->opt;
    if (options) LR_TRY(options_from_public(options, &parsed));
    else parsed.apply_env();
    if (max_batch < 1 || max_batch > 65535) return fail(LR_ERR_ARG, "max_batch must be in 1 .. 65535");
    if (cQ->h.N < 8) return fail(LR_ERR_ARG, "CKKS encryptor: N must be at least 8 (the ternary bit planes hold N / 8 bytes, ring/ternarySampler.go:157)");
    if (cP && cP->device != cQ->device) return fail(LR_ERR_ARG, "contexts live on different devices");
    if (cP && cP->h.N != cQ->h.N) return fail(LR_ERR_ARG, "contexts have different ring degrees");
    std::unique_ptr<lr_ckks_encryptor> e(new lr_ckks_encryptor());
    e->cQ = cQ;
    e->cP = cP;
    e->device = cQ->device;
    e->max_batch = max_batch;
    e->call_by_call = parsed.no_epilogue;
    e->nQ = cQ->h.L();
    e->nP = cP ? cP->h.L() : 0;
    const int rows = e->nQ + e->nP;
    if (rows > kMaxLimbs) return fail(LR_ERR_UNSUPPORTED, "CKKS encryptor: more than 64 limbs in Q||P");
    std::memset(&e->one, 0, sizeof e->one);
    std::memset(&e->minus_one, 0, sizeof e->minus_one);
    for (int i = 0; i < rows; ++i) {     // ring/ring_context.go:119-122
        const HostContext &h = i < e->nQ ? cQ->h : cP->h;
        const int l = i < e->nQ ? i : i - e->nQ;
        e->one.v[i] = mform(1, h.q[l], h.bred[l].hi, h.bred[l].lo);
        e->minus_one.v[i] = mform(h.q[l] - 1, h.q[l], h.bred[l].hi, h.bred[l].lo);
    }
    LR_HIP(hipSetDevice(cQ->device));
    if (cP) LR_TRY(lr_bext_create(cQ, cP, &e->bext));
    LR_HIP(hipMalloc((void **)&e->d_lp, (size_t)rows * sizeof(LimbParams)));
    LR_HIP(hipMemcpy(e->d_lp, cQ->d_lp, (size_t)e->nQ * sizeof(LimbParams), hipMemcpyDeviceToDevice));
    if (cP) LR_HIP(hipMemcpy(e->d_lp + e->nQ, cP->d_lp, (size_t)e->nP * sizeof(LimbParams), hipMemcpyDeviceToDevice));
    const size_t N = (size_t)cQ->h.N, rand_bytes = (size_t)max_batch * (N / 4 + 2 * N);
    LR_HIP(hipMalloc((void **)&e->d_pool, (size_t)3 * max_batch * rows * N * sizeof(u64)));
    LR_HIP(hipMalloc((void **)&e->d_rand, rand_bytes));
    LR_HIP(hipHostMalloc((void **)&e->h_rand, rand_bytes, 0));
    LR_HIP(hipEventCreateWithFlags(&e->staged, hipEventDisableTiming));
    *out = e.release();
    return LR_OK;
    });
}

extern "C" int lr_ckks_encryptor_destroy(lr_ckks_encryptor *e) {
    return guarded([&]() -> int {
    if (!e) return LR_OK;
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();   // the handle's work may be on its context's caller-supplied stream
    delete e;
    return LR_OK;
    });
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
