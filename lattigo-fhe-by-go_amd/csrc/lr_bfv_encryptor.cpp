// lr_bfv_encryptor.cpp -- C ABI: lr_bfv_encryptor and lr_bfv_decryptor, pkEncryptor.encrypt / skEncryptor.encrypt (bfv/encryptor.go:169-223,
// 306-345) and decryptor.Decrypt (bfv/decryptor.go:55-75) for a batch of ciphertexts on the device.  The randomness arrives in the compact
// form the reference's samplers decide before they write limbs and is expanded by the kernels of lr_bfv_encrypt.hip.
// The unit's name keeps it out of the lr_abi_*.cpp set that the shared sanitizer build links against its fixed launch stubs: the launchers
// of lr_bfv_encrypt.hip have a stand-in of their own (tests/cpp/bfv_encryptor_stub.cpp).
#include "lr_host.hpp"

// what newEncryptor builds (bfv/encryptor.go:100-119), plus the staging of the host-randomness entry points
struct lr_bfv_encryptor {
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
    ~lr_bfv_encryptor() {
        for (void *p : {(void *)d_lp, (void *)d_pool, (void *)d_rand})
            if (p) (void)hipFree(p);
        if (h_rand) (void)hipHostFree(h_rand);
        if (staged) (void)hipEventDestroy(staged);
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

struct PkRandom { const unsigned char *u_coeff, *u_sign, *e0, *e1; };

long long key_stride(const lr_poly *p, int batch) { return p->batch == 1 && batch > 1 ? 0 : p->stride(); }

// a poly of the handle's contextQ with at least `limbs` limbs and the call's batch (or, where allowed, one poly for the whole batch)
int check_poly(const lr_bfv_encryptor *e, const lr_poly *p, int limbs, int batch, bool broadcast, const char *what) {
    if (p->ctx != e->cQ) return fail(LR_ERR_ARG, std::string("BFV encryptor: ") + what + " belongs to another context");
    if (p->N != e->cQ->h.N || p->limbs < limbs) return fail(LR_ERR_SHAPE, std::string("BFV encryptor: ") + what + " has too few limbs");
    if (p->batch != batch && !(broadcast && p->batch == 1)) return fail(LR_ERR_SHAPE, std::string("BFV encryptor: batch differs from the batch of ") + what);
    return LR_OK;
}

// everything a call shares: the form against the handle, the outputs, the plaintext
int check_call(const lr_bfv_encryptor *e, int fast, const lr_poly *pt, int batch, const lr_poly *o0, const lr_poly *o1) {
    if (!fast && !e->cP) return fail(LR_ERR_ARG, "BFV encryptor: modulus P is empty -> use the fast form instead (bfv/encryptor.go:123-125)");
    if (o0 == o1 || o0->d == o1->d) return fail(LR_ERR_ARG, "BFV encryptor: the two components of the ciphertext are the same poly");
    if (batch < 1) return fail(LR_ERR_SHAPE, "BFV encryptor: batch must be at least 1");
    if (batch > e->max_batch) return fail(LR_ERR_SHAPE, "batch exceeds the encryptor's max_batch");
    LR_TRY(check_poly(e, pt, e->nQ, batch, true, "the plaintext"));
    LR_TRY(check_poly(e, o0, e->nQ, batch, false, "the ciphertext"));
    LR_TRY(check_poly(e, o1, e->nQ, batch, false, "the ciphertext"));
    if (!fast) LR_TRY(same_stream(e->cQ, e->cP));
    return LR_OK;
}

// the three pool polys of a call, back to back: [3][batch][|Q| + |P|][N]
struct Pools {
    u64 *p[3];
    long long stride, offP;
};
Pools pools_of(const lr_bfv_encryptor *e, int batch) {
    const long long n = (long long)e->cQ->h.N, s = (long long)(e->nQ + e->nP) * n;
    return Pools{{e->d_pool, e->d_pool + batch * s, e->d_pool + 2 * batch * s}, s, (long long)e->nQ * n};
}

// one Context call of contextQP (fast: of contextQ) on rows inside the pools: the Q rows under contextQ, the P rows under contextP
int ewise_qp(lr_bfv_encryptor *e, bool fast, int op, int batch, const u64 *a, long long a_stride, const u64 *b, long long b_stride, u64 *out,
             long long out_stride) {
    const long long offP = (long long)e->nQ * (long long)e->cQ->h.N;
    LR_TRY(run_ewise(e->cQ, op, e->nQ, batch, a, a_stride, b, b_stride, out, out_stride, nullptr));
    if (fast) return LR_OK;
    return run_ewise(e->cP, op, e->nP, batch, a + offP, a_stride, b ? b + offP : nullptr, b_stride, out + offP, out_stride, nullptr);
}

int ntt_qp(lr_bfv_encryptor *e, bool fast, bool inverse, int batch, u64 *in, long long in_stride, u64 *out, long long out_stride) {
    LR_TRY(run_ntt(e->cQ, inverse, Rows{in, in_stride, 0, 1}, Rows{out, out_stride, 0, 1}, 0, 1, e->nQ, batch));
    if (fast) return LR_OK;
    return run_ntt(e->cP, inverse, Rows{in, in_stride, e->nQ, 1}, Rows{out, out_stride, e->nQ, 1}, 0, 1, e->nP, batch);
}

// KYSampler.Sample (ring/gaussianSampler.go:230-251) into a pool poly, from the sampler's bytes
int expand_noise(lr_bfv_encryptor *e, int limbs, int batch, const unsigned char *bytes, u64 *out, long long out_stride) {
    NoiseLaunch L;
    std::memset(&L, 0, sizeof L);
    L.out[0] = out;
    L.out_stride[0] = out_stride;
    L.e[0] = bytes;
    L.n = (int)e->cQ->h.N;
    L.add = 0;
    L.lp = e->d_lp;
    LR_HIP(launch_bfv_noise(L, 1, limbs, batch, e->cQ->stream));
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
    const int n = (int)cQ->h.N, rows = fast ? e->nQ : e->nQ + e->nP;
    const Pools P = pools_of(e, batch);
    const lr_poly *pk[2] = {pk0, pk1};
    lr_poly *outs[2] = {o0, o1};
    const unsigned char *eb[2] = {R.e0, R.e1};
    const long long ps = key_stride(pt, batch);
    {   // :176 / :196 SampleTernaryMontgomeryNTT(polypool[2], 0.5)
        TernaryLaunch T;
        T.coeff_bits = R.u_coeff;
        T.sign_bits = R.u_sign;
        T.out = P.p[2];
        T.out_stride = P.stride;
        T.n = n;
        T.one = e->one;
        T.minus_one = e->minus_one;
        LR_HIP(launch_bfv_ternary(T, rows, batch, cQ->stream));
        LR_TRY(ntt_qp(e, fast, false, batch, P.p[2], P.stride, P.p[2], P.stride));
    }
    if (e->call_by_call) {
        for (int k = 0; k < 2; ++k)      // :178-179 / :200-201 MulCoeffsMontgomery(polypool[2], pk[k], polypool[k])
            LR_TRY(ewise_qp(e, fast, LR_MUL_MONT, batch, P.p[2], P.stride, pk[k]->d, key_stride(pk[k], batch), P.p[k], P.stride));
        for (int k = 0; k < 2; ++k)      // :181-182 / :203-204 InvNTT
            LR_TRY(ntt_qp(e, fast, true, batch, P.p[k], P.stride, P.p[k], P.stride));
        for (int k = 0; k < 2; ++k) {    // :185-190 / :207-212 gaussianSampler.Sample(polypool[2]); Add
            LR_TRY(expand_noise(e, rows, batch, eb[k], P.p[2], P.stride));
            LR_TRY(ewise_qp(e, fast, LR_ADD, batch, P.p[k], P.stride, P.p[2], P.stride, P.p[k], P.stride));
        }
        if (fast) {
            LR_TRY(run_ewise(cQ, LR_ADD, e->nQ, batch, P.p[0], P.stride, pt->d, ps, o0->d, o0->stride(), nullptr));                   // :222
            return run_ewise(cQ, LR_COPY, e->nQ, batch, P.p[1], P.stride, nullptr, 0, o1->d, o1->stride(), nullptr);
        }
        for (int k = 0; k < 2; ++k) LR_TRY(moddown(e, P.p[k], P.stride, batch, outs[k]));                                            // :215-216
        return run_ewise(cQ, LR_ADD, e->nQ, batch, o0->d, o0->stride(), pt->d, ps, o0->d, o0->stride(), nullptr);                    // :222
    }
    {   // both products in one pass over u, all rows of Q||P in one launch
        Mul2Launch M;
        M.a = P.p[2]; M.a_stride = P.stride;
        M.b0 = pk0->d; M.b0_stride = key_stride(pk0, batch);
        M.b1 = pk1->d; M.b1_stride = key_stride(pk1, batch);
        M.out0 = P.p[0]; M.out1 = P.p[1];
        M.out0_stride = M.out1_stride = P.stride;
        M.n = n;
        M.lp = e->d_lp;
        LR_HIP(launch_mul2(M, rows, batch, cQ->stream));
    }
    LR_TRY(ntt_qp(e, fast, true, 2 * batch, P.p[0], P.stride, P.p[0], P.stride));     // the two pools are back to back: one batch of 2 * batch
    NoiseLaunch L;
    std::memset(&L, 0, sizeof L);
    for (int k = 0; k < 2; ++k) {
        L.x[k] = P.p[k];
        L.x_stride[k] = P.stride;
        L.e[k] = eb[k];
        L.out[k] = fast ? outs[k]->d : P.p[k];
        L.out_stride[k] = fast ? outs[k]->stride() : P.stride;
    }
    if (fast) {                          // the Add of the plaintext rides on component 0
        L.plus[0] = pt->d;
        L.plus_stride[0] = ps;
    }
    L.n = n;
    L.add = 1;
    L.lp = e->d_lp;
    LR_HIP(launch_bfv_noise(L, 2, rows, batch, cQ->stream));
    if (fast) return LR_OK;
    for (int k = 0; k < 2; ++k) LR_TRY(moddown(e, P.p[k], P.stride, batch, outs[k]));
    return run_ewise(cQ, LR_ADD, e->nQ, batch, o0->d, o0->stride(), pt->d, ps, o0->d, o0->stride(), nullptr);
}

// skEncryptor.encrypt (bfv/encryptor.go:306-345) after the sampling; crp is read, the reference's in-place InvNTT of it (:331) works on
// its copy in polypool[1] (encryptFromCRP, :296-304)
int encrypt_sk_on_device(lr_bfv_encryptor *e, bool fast, const lr_poly *sk, const lr_poly *crp, const unsigned char *eb, const lr_poly *pt,
                         int batch, lr_poly *o0, lr_poly *o1) {
    lr_context *cQ = e->cQ;
    const int n = (int)cQ->h.N, rows = fast ? e->nQ : e->nQ + e->nP;
    const Pools P = pools_of(e, batch);
    const long long ps = key_stride(pt, batch), ss = key_stride(sk, batch);
    u64 *crp_d = crp->d;
    // fast: the ciphertext's polys take the place of the pool (:314-320)
    u64 *acc = fast ? o0->d : P.p[0], *a_out = fast ? o1->d : P.p[1];
    const long long acc_s = fast ? o0->stride() : P.stride, a_s = fast ? o1->stride() : P.stride;
    if (e->call_by_call) {
        LR_TRY(ewise_qp(e, fast, LR_MUL_MONT, batch, crp_d, crp->stride(), sk->d, ss, acc, acc_s));      // :314 / :326
        LR_TRY(ewise_qp(e, fast, LR_NEG, batch, acc, acc_s, nullptr, 0, acc, acc_s));                    // :315 / :327
        LR_TRY(ntt_qp(e, fast, true, batch, acc, acc_s, acc, acc_s));                                    // :317 / :330
        if (fast) {
            LR_TRY(ntt_qp(e, fast, true, batch, crp_d, crp->stride(), a_out, a_s));                      // :318
        } else {
            LR_TRY(ewise_qp(e, fast, LR_COPY, batch, crp_d, crp->stride(), nullptr, 0, a_out, a_s));     // :300
            LR_TRY(ntt_qp(e, fast, true, batch, a_out, a_s, a_out, a_s));                                // :331
        }
        LR_TRY(expand_noise(e, rows, batch, eb, P.p[2], P.stride));                                      // :320 / :333
        LR_TRY(ewise_qp(e, fast, LR_ADD, batch, acc, acc_s, P.p[2], P.stride, acc, acc_s));
        if (!fast) {
            LR_TRY(moddown(e, P.p[0], P.stride, batch, o0));                                             // :335-336
            LR_TRY(moddown(e, P.p[1], P.stride, batch, o1));
        }
        return run_ewise(cQ, LR_ADD, e->nQ, batch, o0->d, o0->stride(), pt->d, ps, o0->d, o0->stride(), nullptr);   // :344
    }
    NegMulLaunch M;
    M.a = crp_d; M.a_stride = crp->stride();
    M.b = sk->d; M.b_stride = ss;
    M.out = acc; M.out_stride = acc_s;
    M.n = n;
    M.lp = e->d_lp;
    LR_HIP(launch_bfv_negmul(M, rows, batch, cQ->stream));
    LR_TRY(ntt_qp(e, fast, true, batch, acc, acc_s, acc, acc_s));
    LR_TRY(ntt_qp(e, fast, true, batch, crp_d, crp->stride(), a_out, a_s));
    NoiseLaunch L;
    std::memset(&L, 0, sizeof L);
    L.x[0] = L.out[0] = acc;
    L.x_stride[0] = L.out_stride[0] = acc_s;
    L.e[0] = eb;
    if (fast) {                          // the Add of the plaintext rides on the sampler's Add
        L.plus[0] = pt->d;
        L.plus_stride[0] = ps;
    }
    L.n = n;
    L.add = 1;
    L.lp = e->d_lp;
    LR_HIP(launch_bfv_noise(L, 1, rows, batch, cQ->stream));
    if (fast) return LR_OK;
    LR_TRY(moddown(e, P.p[0], P.stride, batch, o0));
    LR_TRY(moddown(e, P.p[1], P.stride, batch, o1));
    return run_ewise(cQ, LR_ADD, e->nQ, batch, o0->d, o0->stride(), pt->d, ps, o0->d, o0->stride(), nullptr);
}

// the caller's bytes through the pinned buffer to the device, pieces one behind the other; the caller's arrays are free on return
int stage_random(lr_bfv_encryptor *e, const unsigned char *const *src, const size_t *bytes, int pieces, const unsigned char **dev) {
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

int encrypt_pk(lr_bfv_encryptor *e, int fast, const lr_poly *pk0, const lr_poly *pk1, const unsigned char *u_coeff, const unsigned char *u_sign,
               const unsigned char *e0, const unsigned char *e1, const lr_poly *pt, int batch, lr_poly *o0, lr_poly *o1, bool on_device) {
    if (!e || !pk0 || !pk1 || !u_coeff || !u_sign || !e0 || !e1 || !pt || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_call(e, fast, pt, batch, o0, o1));
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
    return encrypt_pk_on_device(e, fast != 0, pk0, pk1, R, pt, batch, o0, o1);
}

int encrypt_sk(lr_bfv_encryptor *e, int fast, const lr_poly *sk, const lr_poly *crp, const unsigned char *eb, const lr_poly *pt, int batch,
               lr_poly *o0, lr_poly *o1, bool on_device) {
    if (!e || !sk || !crp || !eb || !pt || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_call(e, fast, pt, batch, o0, o1));
    const int key_limbs = fast ? e->nQ : e->nQ + e->nP;
    LR_TRY(check_poly(e, sk, key_limbs, batch, true, "the secret key"));
    LR_TRY(check_poly(e, crp, key_limbs, batch, false, "the uniform poly"));
    if (crp->d == o0->d || crp->d == o1->d) return fail(LR_ERR_ARG, "BFV encryptor: the uniform poly is not modified and cannot be an output");
    LR_HIP(hipSetDevice(e->device));
    if (!on_device) {
        const unsigned char *src[1] = {eb}, *dev[1];
        const size_t bytes[1] = {(size_t)batch * (size_t)e->cQ->h.N};
        LR_TRY(stage_random(e, src, bytes, 1, dev));
        eb = dev[0];
    }
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
    Options parsed = cQ->opt;
    if (options) LR_TRY(options_from_public(options, &parsed));
    else parsed.apply_env();
    if (max_batch < 1 || max_batch > 65535) return fail(LR_ERR_ARG, "max_batch must be in 1 .. 65535");
    if (cQ->h.N < 8) return fail(LR_ERR_ARG, "BFV encryptor: N must be at least 8 (the ternary bit planes hold N / 8 bytes, ring/ternarySampler.go:157)");
    if (cP && cP->device != cQ->device) return fail(LR_ERR_ARG, "contexts live on different devices");
    if (cP && cP->h.N != cQ->h.N) return fail(LR_ERR_ARG, "contexts have different ring degrees");
    std::unique_ptr<lr_bfv_encryptor> e(new lr_bfv_encryptor());
    e->cQ = cQ;
    e->cP = cP;
    e->device = cQ->device;
    e->max_batch = max_batch;
    e->call_by_call = parsed.no_epilogue;
    e->nQ = cQ->h.L();
    e->nP = cP ? cP->h.L() : 0;
    const int rows = e->nQ + e->nP;
    if (rows > kMaxLimbs) return fail(LR_ERR_UNSUPPORTED, "BFV encryptor: more than 64 limbs in Q||P");
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

extern "C" int lr_bfv_encryptor_destroy(lr_bfv_encryptor *e) {
    return guarded([&]() -> int {
    if (!e) return LR_OK;
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();   // the handle's work may be on its context's caller-supplied stream
    delete e;
    return LR_OK;
    });
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
