// lr_keygen.cpp -- C ABI: lr_keygen, the KeyGenerator of ckks/keygen.go and bfv/keygen.go for a batch of keys on the device: GenSecretKey,
// GenPublicKey, newSwitchingKey and what GenRelinKey, GenSwitchingKey and genrotKey put in front of it.  The randomness arrives in the
// compact form of the encryptors (lr_bfv_encryptor); the uniform halves are the caller's polys.  Kernels: lr_keygen.hip and the expansion
// of lr_ckks_encrypt.hip.
// The unit's name keeps it out of the lr_abi_*.cpp set that the shared sanitizer build links against its fixed launch stubs: the launchers
// it calls have a stand-in of their own (tests/cpp/keygen_stub.cpp).  That is why the extern "C" entry points live here and not in a
// lr_abi_keygen.cpp.
#include "lr_host.hpp"

// what NewKeyGenerator builds (ckks/keygen.go:79-94), plus the staging of the host-randomness entry points
struct lr_keygen {
    int device = 0;
    lr_context *cQ = nullptr, *cP = nullptr;  // cP == nullptr: "modulus P is empty", only the secret key and the public key
    int nQ = 0, nP = 0, alpha = 0, beta = 0, max_batch = 0, chunk = 0;   // chunk: keys per pass, min(max_batch, kKeygenKeysPerLaunch)
    bool call_by_call = false;                // Options::no_epilogue: the reference's call-by-call shape
    LimbScalars one, minus_one;               // matrixTernaryMontgomery rows 1 and 2 (ring/ring_context.go:119-122) per limb of Q||P
    LimbScalars pmont;                        // MForm(P mod q_j) per limb of Q: MulScalarBigint's scalar (ring/ring.go:547)
    LimbParams *d_lp = nullptr;               // the limb constants of contextQP: contextQ's, then contextP's
    u64 *d_pool = nullptr;                    // chunk * beta noise polys over Q||P, then chunk skIn polys over Q
    unsigned char *d_rand = nullptr;          // the host-randomness entry points' bytes on the device ...
    unsigned char *h_rand = nullptr;          // ... and pinned: max_batch * max(beta, 1) * N
    hipEvent_t staged = nullptr;              // the last copy out of h_rand: the next call waits for it before it refills the buffer
    ~lr_keygen() {
        for (void *p : {(void *)d_lp, (void *)d_pool, (void *)d_rand})
            if (p) (void)hipFree(p);
        if (h_rand) (void)hipHostFree(h_rand);
        if (staged) (void)hipEventDestroy(staged);
    }
};

namespace lr_host {
namespace {

enum SkInKind { SkInPlain, SkInRotation, SkInPowers };

long long shared_stride(const lr_poly *p, int batch) { return p->batch == 1 && batch > 1 ? 0 : p->stride(); }

// a poly of the handle's contextQ over all of Q||P with the given batch (or, where allowed, one poly for the whole batch)
int check_poly(const lr_keygen *g, const lr_poly *p, int batch, bool broadcast, const char *what) {
    if (p->ctx != g->cQ) return fail(LR_ERR_ARG, std::string("key generator: ") + what + " belongs to another context");
    if (p->N != g->cQ->h.N || p->limbs < g->nQ + g->nP) return fail(LR_ERR_SHAPE, std::string("key generator: ") + what + " has too few limbs");
    if (p->batch != batch && !(broadcast && p->batch == 1)) return fail(LR_ERR_SHAPE, std::string("key generator: batch differs from the batch of ") + what);
    return LR_OK;
}

// the words of two polys overlap: an output that is, or lies inside, an input
bool overlap(const lr_poly *a, const lr_poly *b) {
    const u64 *a1 = a->d + (long long)(a->batch - 1) * a->stride() + (long long)a->alloc_limbs * (long long)a->N;
    const u64 *b1 = b->d + (long long)(b->batch - 1) * b->stride() + (long long)b->alloc_limbs * (long long)b->N;
    return a->d < b1 && b->d < a1;
}

int check_batch(const lr_keygen *g, int batch, const char *what) {
    if (batch < 1) return fail(LR_ERR_SHAPE, std::string("key generator: ") + what + " must be at least 1");
    if (batch > g->max_batch) return fail(LR_ERR_SHAPE, std::string("key generator: ") + what + " exceeds the key generator's max_batch");
    return LR_OK;
}

// one Context call of contextQP on `batch` polys: the Q rows under contextQ, the P rows under contextP
int ewise_qp(lr_keygen *g, int op, int batch, const u64 *a, long long a_stride, const u64 *b, long long b_stride, u64 *out, long long out_stride) {
    const long long offP = (long long)g->nQ * (long long)g->cQ->h.N;
    LR_TRY(run_ewise(g->cQ, op, g->nQ, batch, a, a_stride, b, b_stride, out, out_stride, nullptr));
    if (!g->cP) return LR_OK;
    return run_ewise(g->cP, op, g->nP, batch, a + offP, a_stride, b ? b + offP : nullptr, b_stride, out + offP, out_stride, nullptr);
}

// Context.NTT of contextQP in place on `items` polys: the route lr_ntt picks, batched over the items
int ntt_qp(lr_keygen *g, u64 *p, long long stride, int items) {
    LR_TRY(run_ntt(g->cQ, false, Rows{p, stride, 0, 1}, Rows{p, stride, 0, 1}, 0, 1, g->nQ, items));
    if (!g->cP) return LR_OK;
    return run_ntt(g->cP, false, Rows{p, stride, g->nQ, 1}, Rows{p, stride, g->nQ, 1}, 0, 1, g->nP, items);
}

// SampleTernaryMontgomery (ternary) or KYSampler.Sample (noise) into `items` polys over Q||P, then Context.NTT: the transform's operand
// keeps the 0 of (0, sign 0), which the transform's last reduction gives anyway
int sample_ntt(lr_keygen *g, const unsigned char *coeff_bits, const unsigned char *sign_bits, const unsigned char *eb, u64 *out, long long stride,
               int items) {
    CkksExpandLaunch X;
    std::memset(&X, 0, sizeof X);
    X.coeff_bits = coeff_bits;
    X.sign_bits = sign_bits;
    X.e[0] = eb;
    X.out = out;
    X.out_stride = stride;
    X.n = (int)g->cQ->h.N;
    X.ternary = eb ? 0 : 1;
    X.noises = eb ? 1 : 0;
    X.one = g->one;
    X.minus_one = g->minus_one;
    X.lp = g->d_lp;
    LR_HIP(launch_ckks_expand(X, g->nQ + g->nP, items, g->cQ->stream));
    return ntt_qp(g, out, stride, items);
}

// the caller's bytes through the pinned buffer to the device, pieces one behind the other; the caller's arrays are free on return
int stage_random(lr_keygen *g, const unsigned char *const *src, const size_t *bytes, int pieces, const unsigned char **dev) {
    LR_HIP(hipEventSynchronize(g->staged));               // the copy of the call before has left the pinned buffer
    size_t off = 0;
    for (int i = 0; i < pieces; ++i) {
        std::memcpy(g->h_rand + off, src[i], bytes[i]);
        dev[i] = g->d_rand + off;
        off += bytes[i];
    }
    LR_HIP(hipMemcpyAsync(g->d_rand, g->h_rand, off, hipMemcpyHostToDevice, g->cQ->stream));
    LR_HIP(hipEventRecord(g->staged, g->cQ->stream));
    return LR_OK;
}

// GenSecretKey (ckks/keygen.go:97-106): SampleTernaryMontgomeryNTTNew over contextQP
int secret_key(lr_keygen *g, const unsigned char *coeff_bits, const unsigned char *sign_bits, int batch, lr_poly *sk, bool on_device) {
    if (!g || !coeff_bits || !sign_bits || !sk) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_batch(g, batch, "batch"));
    LR_TRY(check_poly(g, sk, batch, false, "the secret key"));
    if (g->cP) LR_TRY(same_stream(g->cQ, g->cP));       // the P rows are transformed under contextP
    LR_HIP(hipSetDevice(g->device));
    if (!on_device) {
        const size_t plane = (size_t)batch * (size_t)(g->cQ->h.N >> 3);
        const unsigned char *src[2] = {coeff_bits, sign_bits}, *dev[2];
        const size_t bytes[2] = {plane, plane};
        LR_TRY(stage_random(g, src, bytes, 2, dev));
        coeff_bits = dev[0];
        sign_bits = dev[1];
    }
    return sample_ntt(g, coeff_bits, sign_bits, nullptr, sk->d, sk->stride(), batch);
}

// GenPublicKey (ckks/keygen.go:138-151, bfv/keygen.go:121-136); pk1 is the caller's uniform poly
int public_key(lr_keygen *g, const lr_poly *sk, const unsigned char *eb, int batch, lr_poly *pk0, const lr_poly *pk1, bool on_device) {
    if (!g || !sk || !eb || !pk0 || !pk1) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_batch(g, batch, "batch"));
    LR_TRY(check_poly(g, sk, batch, true, "the secret key"));
    LR_TRY(check_poly(g, pk1, batch, false, "the uniform poly"));
    LR_TRY(check_poly(g, pk0, batch, false, "the public key"));
    if (overlap(pk0, sk) || overlap(pk0, pk1)) return fail(LR_ERR_ARG, "key generator: the public key's output is one of its inputs");
    if (g->cP) LR_TRY(same_stream(g->cQ, g->cP));
    LR_HIP(hipSetDevice(g->device));
    if (!on_device) {
        const unsigned char *src[1] = {eb}, *dev[1];
        const size_t bytes[1] = {(size_t)batch * (size_t)g->cQ->h.N};
        LR_TRY(stage_random(g, src, bytes, 1, dev));
        eb = dev[0];
    }
    LR_TRY(sample_ntt(g, nullptr, nullptr, eb, pk0->d, pk0->stride(), batch));                                       // :144 SampleNTTNew
    const long long ss = shared_stride(sk, batch);
    if (g->call_by_call) {
        LR_TRY(ewise_qp(g, LR_MUL_MONT_AND_ADD, batch, sk->d, ss, pk1->d, pk1->stride(), pk0->d, pk0->stride()));    // :147
        return ewise_qp(g, LR_NEG, batch, pk0->d, pk0->stride(), nullptr, 0, pk0->d, pk0->stride());                 // :148
    }
    KeygenPkLaunch L;
    L.sk = sk->d; L.sk_stride = ss;
    L.pk1 = pk1->d; L.pk1_stride = pk1->stride();
    L.pk0 = pk0->d; L.pk0_stride = pk0->stride();
    L.n = (int)g->cQ->h.N;
    L.lp = g->d_lp;
    LR_HIP(launch_keygen_pk(L, g->nQ + g->nP, batch, g->cQ->stream));
    return LR_OK;
}

// digit i owns rows [d0, d1) of Q: the loop of ckks/keygen.go:315-331 with its break
void digit_rows(const lr_keygen *g, int i, int *d0, int *d1) {
    *d0 = i * g->alpha;
    *d1 = std::min((i + 1) * g->alpha, g->nQ);
}

// skIn of keys [first, first + keys) in the reference's call-by-call shape, one key at a time
int skin_call_by_call(lr_keygen *g, SkInKind kind, const lr_poly *sk_in, long long in_stride, const u64 *gens, int first, int keys, u64 *skin,
                      long long skin_stride) {
    lr_context *cQ = g->cQ;
    for (int k = 0; k < keys; ++k) {
        u64 *out = skin + k * skin_stride;
        const u64 *in = sk_in->d + (long long)(first + k) * in_stride;
        if (kind == SkInRotation) {
            LR_TRY(run_permute_ntt(cQ, g->nQ, 1, in, 0, out, 0, gens[first + k]));                                   // genrotKey, ckks/keygen.go:489
            LR_TRY(run_ewise(cQ, LR_MUL_SCALAR_LIMBS, g->nQ, 1, out, 0, nullptr, 0, out, 0, &g->pmont));             // :290
        } else if (kind == SkInPlain) {
            LR_TRY(run_ewise(cQ, LR_MUL_SCALAR_LIMBS, g->nQ, 1, in, 0, nullptr, 0, out, 0, &g->pmont));              // bfv/keygen.go:255
        } else if (k > 0) {
            LR_TRY(run_ewise(cQ, LR_MUL_MONT, g->nQ, 1, out - skin_stride, 0, sk_in->d, 0, out, 0, nullptr));        // bfv/keygen.go:189
        } else {
            LR_TRY(run_ewise(cQ, LR_MUL_SCALAR_LIMBS, g->nQ, 1, sk_in->d, 0, nullptr, 0, out, 0, &g->pmont));        // bfv/keygen.go:186
            for (int p = 0; p <= first; ++p) LR_TRY(run_ewise(cQ, LR_MUL_MONT, g->nQ, 1, out, 0, sk_in->d, 0, out, 0, nullptr));
        }
    }
    return LR_OK;
}

// newSwitchingKey (ckks/keygen.go:282-338, bfv/keygen.go:285-333) for n_keys keys, with what its callers do to skIn first.  The two
// schemes' lines give the same bits (tests/test_oracle_keygen.py), so one path serves both.
int switching_keys(lr_keygen *g, SkInKind kind, const lr_poly *sk_in, const lr_poly *sk_out, const u64 *gens, const unsigned char *eb, int n_keys,
                   lr_poly *const *evks, bool on_device) {
    if (!g || !sk_in || !sk_out || !eb || !evks || (kind == SkInRotation && !gens)) return fail(LR_ERR_ARG, "null argument");
    if (!g->cP) return fail(LR_ERR_ARG, "key generator: modulus P is empty (ckks/keygen.go:249-251)");
    LR_TRY(check_batch(g, n_keys, kind == SkInPowers ? "n_powers" : "n_keys"));
    const int rows = g->nQ + g->nP, beta = g->beta;
    LR_TRY(check_poly(g, sk_out, n_keys, true, "the output secret key"));
    if (kind == SkInPlain) LR_TRY(check_poly(g, sk_in, n_keys, true, "the input secret key"));
    else if (sk_out->batch != 1) return fail(LR_ERR_SHAPE, "key generator: relinearisation and rotation keys take one secret key");
    for (int k = 0; k < n_keys; ++k) {
        if (!evks[k]) return fail(LR_ERR_ARG, "null argument");
        if (evks[k]->ctx != g->cQ) return fail(LR_ERR_ARG, "key generator: a switching key belongs to another context");
        if (evks[k]->N != g->cQ->h.N || evks[k]->limbs < rows) return fail(LR_ERR_SHAPE, "key generator: a switching key has too few limbs");
        if (evks[k]->batch != 2 * beta) return fail(LR_ERR_SHAPE, "key generator: a switching key's batch is not 2 beta");
        if (overlap(evks[k], sk_in) || overlap(evks[k], sk_out)) return fail(LR_ERR_ARG, "key generator: a switching key is one of the secret keys");
        for (int j = 0; j < k; ++j)
            if (overlap(evks[k], evks[j])) return fail(LR_ERR_ARG, "key generator: two switching keys share memory");
        if (kind == SkInRotation && !(gens[k] & 1)) return fail(LR_ERR_ARG, "key generator: a Galois element is even");
    }
    LR_TRY(same_stream(g->cQ, g->cP));
    LR_HIP(hipSetDevice(g->device));
    lr_context *cQ = g->cQ;
    const long long n = (long long)cQ->h.N, e_stride = rows * n, skin_stride = g->nQ * n;
    if (!on_device) {
        const unsigned char *src[1] = {eb}, *dev[1];
        const size_t bytes[1] = {(size_t)n_keys * (size_t)beta * (size_t)n};
        LR_TRY(stage_random(g, src, bytes, 1, dev));
        eb = dev[0];
    }
    u64 *pool_e = g->d_pool, *skin = g->d_pool + (long long)g->chunk * beta * e_stride;
    const long long in_stride = kind == SkInPlain ? shared_stride(sk_in, n_keys) : 0, out_key_stride = shared_stride(sk_out, n_keys);
    const u64 mask2 = 2 * (u64)n - 1;
    for (int first = 0; first < n_keys; first += g->chunk) {
        const int keys = std::min(g->chunk, n_keys - first), items = keys * beta;
        LR_TRY(sample_ntt(g, nullptr, nullptr, eb + (long long)first * beta * n, pool_e, e_stride, items));          // :302 SampleNTTNew, every digit
        const u64 *skout = sk_out->d + first * out_key_stride;
        if (g->call_by_call) {
            LR_TRY(skin_call_by_call(g, kind, sk_in, in_stride, gens, first, keys, skin, skin_stride));
            for (int k = 0; k < keys; ++k)
                for (int i = 0; i < beta; ++i) {
                    const u64 *e = pool_e + (long long)(k * beta + i) * e_stride;
                    const lr_poly *key = evks[first + k];
                    u64 *even = key->d + (long long)(2 * i) * key->stride();
                    const u64 *odd = key->d + (long long)(2 * i + 1) * key->stride();
                    int d0, d1;
                    digit_rows(g, i, &d0, &d1);
                    LR_TRY(ewise_qp(g, LR_MFORM, 1, e, 0, nullptr, 0, even, 0));                                      // :303
                    LR_TRY(run_ewise(cQ, LR_ADD, d1 - d0, 1, even + d0 * n, 0, skin + k * skin_stride + d0 * n, 0, even + d0 * n, 0, nullptr, d0));   // :315-331
                    LR_TRY(ewise_qp(g, LR_MUL_MONT_AND_SUB, 1, odd, 0, skout + k * out_key_stride, 0, even, 0));      // :334
                }
            continue;
        }
        if (kind == SkInPowers) {
            KeygenPowersLaunch S;
            S.sk = sk_in->d;
            S.out = skin;
            S.out_stride = skin_stride;
            S.n = (int)n;
            S.first = first;
            S.keys = keys;
            S.pmont = g->pmont;
            S.lp = g->d_lp;
            LR_HIP(launch_keygen_powers(S, g->nQ, cQ->stream));
        } else {
            KeygenSkInLaunch S;
            std::memset(&S, 0, sizeof S);
            S.sk = sk_in->d + first * in_stride;
            S.sk_stride = in_stride;
            S.out = skin;
            S.out_stride = skin_stride;
            for (int k = 0; k < keys; ++k) S.gen[k] = kind == SkInRotation ? (u32)(gens[first + k] & mask2) : 1u;
            S.n = (int)n;
            S.logn = (int)cQ->h.logN;
            S.pmont = g->pmont;
            S.lp = g->d_lp;
            LR_HIP(launch_keygen_skin(S, g->nQ, keys, cQ->stream));
        }
        KeygenFinishLaunch F;
        std::memset(&F, 0, sizeof F);
        F.e = pool_e; F.e_stride = e_stride;
        F.skin = skin; F.skin_stride = skin_stride;
        F.skout = skout; F.skout_stride = out_key_stride;
        for (int k = 0; k < keys; ++k) F.key[k] = KeygenKeyRef{evks[first + k]->d, evks[first + k]->stride()};
        F.n = (int)n;
        F.nQ = g->nQ;
        F.alpha = g->alpha;
        F.beta = beta;
        F.lp = g->d_lp;
        LR_HIP(launch_keygen_finish(F, rows, keys, cQ->stream));
    }
    return LR_OK;
}

}  // namespace
}  // namespace lr_host

extern "C" int lr_keygen_create(lr_context *cQ, lr_context *cP, int max_batch, lr_keygen **out) {
    return lr_keygen_create_ex(cQ, cP, max_batch, nullptr, out);
}

extern "C" int lr_keygen_create_ex(lr_context *cQ, lr_context *cP, int max_batch, const lr_options *options, lr_keygen **out) {
    return guarded([&]() -> int {
    if (!cQ || !out) return fail(LR_ERR_ARG, "null argument");
    *out = nullptr;
    Options parsed = cQ->opt;
    if (options) LR_TRY(options_from_public(options, &parsed));
    else parsed.apply_env();
    if (max_batch < 1 || max_batch > 65535) return fail(LR_ERR_ARG, "max_batch must be in 1 .. 65535");
    if (cQ->h.N < 8) return fail(LR_ERR_ARG, "key generator: N must be at least 8 (the ternary bit planes hold N / 8 bytes, ring/ternarySampler.go:157)");
    if (cQ->h.logN > 30) return fail(LR_ERR_UNSUPPORTED, "key generator: ring degree");
    if (cP && cP->device != cQ->device) return fail(LR_ERR_ARG, "contexts live on different devices");
    if (cP && cP->h.N != cQ->h.N) return fail(LR_ERR_ARG, "contexts have different ring degrees");
    std::unique_ptr<lr_keygen> g(new lr_keygen());
    g->cQ = cQ;
    g->cP = cP;
    g->device = cQ->device;
    g->max_batch = max_batch;
    g->chunk = std::min(max_batch, kKeygenKeysPerLaunch);
    g->call_by_call = parsed.no_epilogue;
    g->nQ = cQ->h.L();
    g->nP = cP ? cP->h.L() : 0;
    g->alpha = g->nP;                                                // params.Alpha() = |P|, Beta() = ceil(|Q| / |P|)
    g->beta = cP ? (g->nQ + g->nP - 1) / g->nP : 0;
    const int rows = g->nQ + g->nP;
    if (rows > kMaxLimbs) return fail(LR_ERR_UNSUPPORTED, "key generator: more than 64 limbs in Q||P");
    std::memset(&g->one, 0, sizeof g->one);
    std::memset(&g->minus_one, 0, sizeof g->minus_one);
    std::memset(&g->pmont, 0, sizeof g->pmont);
    for (int i = 0; i < rows; ++i) {     // ring/ring_context.go:119-122
        const HostContext &h = i < g->nQ ? cQ->h : cP->h;
        const int l = i < g->nQ ? i : i - g->nQ;
        g->one.v[i] = mform(1, h.q[l], h.bred[l].hi, h.bred[l].lo);
        g->minus_one.v[i] = mform(h.q[l] - 1, h.q[l], h.bred[l].hi, h.bred[l].lo);
    }
    for (int i = 0; cP && i < g->nQ; ++i) {   // contextP.ModulusBigint mod q_i, then MForm (ring/ring.go:545-547)
        const u64 q = cQ->h.q[i];
        u64 p = 1 % q;
        for (int j = 0; j < g->nP; ++j) p = (u64)(((u128)p * (cP->h.q[j] % q)) % q);
        g->pmont.v[i] = mform(p, q, cQ->h.bred[i].hi, cQ->h.bred[i].lo);
    }
    LR_HIP(hipSetDevice(cQ->device));
    LR_HIP(hipMalloc((void **)&g->d_lp, (size_t)rows * sizeof(LimbParams)));
    LR_HIP(hipMemcpy(g->d_lp, cQ->d_lp, (size_t)g->nQ * sizeof(LimbParams), hipMemcpyDeviceToDevice));
    if (cP) LR_HIP(hipMemcpy(g->d_lp + g->nQ, cP->d_lp, (size_t)g->nP * sizeof(LimbParams), hipMemcpyDeviceToDevice));
    const size_t N = (size_t)cQ->h.N, rand_bytes = (size_t)max_batch * (size_t)std::max(g->beta, 1) * N;
    if (cP) LR_HIP(hipMalloc((void **)&g->d_pool, (size_t)g->chunk * ((size_t)g->beta * rows + g->nQ) * N * sizeof(u64)));
    LR_HIP(hipMalloc((void **)&g->d_rand, rand_bytes));
    LR_HIP(hipHostMalloc((void **)&g->h_rand, rand_bytes, 0));
    LR_HIP(hipEventCreateWithFlags(&g->staged, hipEventDisableTiming));
    *out = g.release();
    return LR_OK;
    });
}

extern "C" int lr_keygen_destroy(lr_keygen *g) {
    return guarded([&]() -> int {
    if (!g) return LR_OK;
    (void)hipSetDevice(g->device);
    (void)hipDeviceSynchronize();   // the handle's work may be on its context's caller-supplied stream
    delete g;
    return LR_OK;
    });
}

typedef const unsigned char *bytes_t;

extern "C" int lr_keygen_secret_key(lr_keygen *g, const uint8_t *coeff_bits, const uint8_t *sign_bits, int batch, lr_poly *sk_out) {
    return guarded([&]() -> int { return secret_key(g, coeff_bits, sign_bits, batch, sk_out, false); });
}
extern "C" int lr_keygen_secret_key_device(lr_keygen *g, const void *coeff_bits, const void *sign_bits, int batch, lr_poly *sk_out) {
    return guarded([&]() -> int { return secret_key(g, (bytes_t)coeff_bits, (bytes_t)sign_bits, batch, sk_out, true); });
}
extern "C" int lr_keygen_public_key(lr_keygen *g, const lr_poly *sk, const uint8_t *e, int batch, lr_poly *pk0_out, const lr_poly *pk1) {
    return guarded([&]() -> int { return public_key(g, sk, e, batch, pk0_out, pk1, false); });
}
extern "C" int lr_keygen_public_key_device(lr_keygen *g, const lr_poly *sk, const void *e, int batch, lr_poly *pk0_out, const lr_poly *pk1) {
    return guarded([&]() -> int { return public_key(g, sk, (bytes_t)e, batch, pk0_out, pk1, true); });
}
extern "C" int lr_keygen_switching_keys(lr_keygen *g, const lr_poly *sk_in, const lr_poly *sk_out, const uint8_t *e, int n_keys, lr_poly *const *evks) {
    return guarded([&]() -> int { return switching_keys(g, SkInPlain, sk_in, sk_out, nullptr, e, n_keys, evks, false); });
}
extern "C" int lr_keygen_switching_keys_device(lr_keygen *g, const lr_poly *sk_in, const lr_poly *sk_out, const void *e, int n_keys,
                                               lr_poly *const *evks) {
    return guarded([&]() -> int { return switching_keys(g, SkInPlain, sk_in, sk_out, nullptr, (bytes_t)e, n_keys, evks, true); });
}
extern "C" int lr_keygen_relin_keys(lr_keygen *g, const lr_poly *sk, int n_powers, const uint8_t *e, lr_poly *const *evks) {
    return guarded([&]() -> int { return switching_keys(g, SkInPowers, sk, sk, nullptr, e, n_powers, evks, false); });
}
extern "C" int lr_keygen_relin_keys_device(lr_keygen *g, const lr_poly *sk, int n_powers, const void *e, lr_poly *const *evks) {
    return guarded([&]() -> int { return switching_keys(g, SkInPowers, sk, sk, nullptr, (bytes_t)e, n_powers, evks, true); });
}
extern "C" int lr_keygen_rotation_keys(lr_keygen *g, const lr_poly *sk, const uint64_t *galois_elements, int n_keys, const uint8_t *e,
                                       lr_poly *const *evks) {
    return guarded([&]() -> int { return switching_keys(g, SkInRotation, sk, sk, galois_elements, e, n_keys, evks, false); });
}
extern "C" int lr_keygen_rotation_keys_device(lr_keygen *g, const lr_poly *sk, const uint64_t *galois_elements, int n_keys, const void *e,
                                              lr_poly *const *evks) {
    return guarded([&]() -> int { return switching_keys(g, SkInRotation, sk, sk, galois_elements, (bytes_t)e, n_keys, evks, true); });
}
