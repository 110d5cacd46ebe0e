// lr_keygen.cpp -- C ABI: lr_keygen, the KeyGenerator of ckks/keygen.go and bfv/keygen.go for a batch of keys on the device: GenSecretKey,
// GenPublicKey, newSwitchingKey and what GenRelinKey, GenSwitchingKey and genrotKey put in front of it.  The randomness arrives in the
// compact form of the encryptors (lr_bfv_encryptor); the uniform halves are the caller's polys.  Kernels: lr_keygen.hip and the expansion
// of lr_ckks_encrypt.hip.
// The host sanitizer build (tests/host_stub_build.py) compiles this unit with every other; the launchers of lr_keygen.hip have their
// stand-in in tests/cpp/hipstub/stub_keygen.cpp.  The extern "C" entry points live here, beside the handle.  What it shares with the
// encryptors and lr_collective.cpp is lr_qp_handle.hpp.
#include "lr_qp_handle.hpp"

// what NewKeyGenerator builds (ckks/keygen.go:79-94); the contexts, the scalars and the staging of the host-randomness entry points
// (max_batch * max(beta, 1) * N bytes) are QpHandle's.  cP == nullptr: only the secret key and the public key
struct lr_keygen : lr_host::QpHandle {
    int alpha = 0, beta = 0, chunk = 0;       // chunk: keys per pass, min(max_batch, kKeygenKeysPerLaunch)
    u64 *d_pool = nullptr;                    // chunk * beta noise polys over Q||P, then chunk skIn polys over Q
    ~lr_keygen() {
        if (d_pool) (void)hipFree(d_pool);
    }
};

namespace lr_host {
namespace {

enum SkInKind { SkInPlain, SkInRotation, SkInPowers };

int check_batch(const lr_keygen *g, int batch, const char *what) {
    if (batch < 1) return fail(LR_ERR_SHAPE, std::string("key generator: ") + what + " must be at least 1");
    if (batch > g->max_batch) return fail(LR_ERR_SHAPE, std::string("key generator: ") + what + " exceeds the key generator's max_batch");
    return LR_OK;
}

// SampleTernaryMontgomery (ternary) or KYSampler.Sample (noise) into `items` polys over Q||P, then Context.NTT (the route lr_ntt picks,
// batched over the items): the transform's operand keeps the 0 of (0, sign 0), which the transform's last reduction gives anyway
int sample_ntt(lr_keygen *g, const unsigned char *coeff_bits, const unsigned char *sign_bits, const unsigned char *eb, u64 *out, long long stride,
               int items) {
    LR_TRY(expand_qp(g, 0, g->rows(), eb ? 0 : 1, coeff_bits, sign_bits, eb ? 1 : 0, eb, nullptr, out, stride, 0, items));
    return ntt_qp(g, g->cP != nullptr, false, g->nQ, items, out, stride, out, stride);
}

// GenSecretKey (ckks/keygen.go:97-106): SampleTernaryMontgomeryNTTNew over contextQP
int secret_key(lr_keygen *g, const unsigned char *coeff_bits, const unsigned char *sign_bits, int batch, lr_poly *sk, bool on_device) {
    if (!g || !coeff_bits || !sign_bits || !sk) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_batch(g, batch, "batch"));
    LR_TRY(g->check_poly(sk, g->rows(), batch, false, "the secret key"));
    if (g->cP) LR_TRY(same_stream(g->cQ, g->cP));       // the P rows are transformed under contextP
    LR_HIP(hipSetDevice(g->device));
    if (!on_device) {
        const size_t plane = (size_t)batch * (size_t)(g->cQ->h.N >> 3);
        const unsigned char *src[2] = {coeff_bits, sign_bits}, *dev[2];
        const size_t bytes[2] = {plane, plane};
        LR_TRY(g->stage_random(src, bytes, 2, dev));
        coeff_bits = dev[0];
        sign_bits = dev[1];
    }
    return sample_ntt(g, coeff_bits, sign_bits, nullptr, sk->d, sk->stride(), batch);
}

// GenPublicKey (ckks/keygen.go:138-151, bfv/keygen.go:121-136); pk1 is the caller's uniform poly
int public_key(lr_keygen *g, const lr_poly *sk, const unsigned char *eb, int batch, lr_poly *pk0, const lr_poly *pk1, bool on_device) {
    if (!g || !sk || !eb || !pk0 || !pk1) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_batch(g, batch, "batch"));
    LR_TRY(g->check_poly(sk, g->rows(), batch, true, "the secret key"));
    LR_TRY(g->check_poly(pk1, g->rows(), batch, false, "the uniform poly"));
    LR_TRY(g->check_poly(pk0, g->rows(), batch, false, "the public key"));
    if (overlap(pk0, sk) || overlap(pk0, pk1)) return fail(LR_ERR_ARG, "key generator: the public key's output is one of its inputs");
    if (g->cP) LR_TRY(same_stream(g->cQ, g->cP));
    LR_HIP(hipSetDevice(g->device));
    if (!on_device) LR_TRY(g->stage_random(&eb, (size_t)batch * (size_t)g->cQ->h.N));
    LR_TRY(sample_ntt(g, nullptr, nullptr, eb, pk0->d, pk0->stride(), batch));                                       // :144 SampleNTTNew
    const long long ss = key_stride(sk, batch);
    if (g->call_by_call) {
        LR_TRY(ewise_qp(g, g->cP != nullptr, LR_MUL_MONT_AND_ADD, batch, sk->d, ss, pk1->d, pk1->stride(), pk0->d, pk0->stride()));    // :147
        return ewise_qp(g, g->cP != nullptr, LR_NEG, batch, pk0->d, pk0->stride(), nullptr, 0, pk0->d, pk0->stride());                 // :148
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
    LR_TRY(g->check_poly(sk_out, g->rows(), n_keys, true, "the output secret key"));
    if (kind == SkInPlain) LR_TRY(g->check_poly(sk_in, g->rows(), n_keys, true, "the input secret key"));
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
    if (!on_device) LR_TRY(g->stage_random(&eb, (size_t)n_keys * (size_t)beta * (size_t)n));
    u64 *pool_e = g->d_pool, *skin = g->d_pool + (long long)g->chunk * beta * e_stride;
    const long long in_stride = kind == SkInPlain ? key_stride(sk_in, n_keys) : 0, out_key_stride = key_stride(sk_out, n_keys);
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
                    LR_TRY(ewise_qp(g, true, LR_MFORM, 1, e, 0, nullptr, 0, even, 0));                                                 // :303
                    LR_TRY(run_ewise(cQ, LR_ADD, d1 - d0, 1, even + d0 * n, 0, skin + k * skin_stride + d0 * n, 0, even + d0 * n, 0, nullptr, d0));   // :315-331
                    LR_TRY(ewise_qp(g, true, LR_MUL_MONT_AND_SUB, 1, odd, 0, skout + k * out_key_stride, 0, even, 0));                 // :334
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
    const char *name = "key generator";
    Options parsed;
    LR_TRY(check_create(name, cQ, max_batch, options, &parsed));
    if (cQ->h.logN > 30) return fail(LR_ERR_UNSUPPORTED, "key generator: ring degree");
    LR_TRY(check_pair(cQ, cP));
    std::unique_ptr<lr_keygen> g(new lr_keygen());
    LR_TRY(g->init(name, cQ, cP, max_batch, parsed));
    g->chunk = std::min(max_batch, kKeygenKeysPerLaunch);
    g->alpha = g->nP;                                                // params.Alpha() = |P|, Beta() = ceil(|Q| / |P|)
    g->beta = cP ? (g->nQ + g->nP - 1) / g->nP : 0;
    LR_HIP(hipSetDevice(cQ->device));
    const size_t N = (size_t)cQ->h.N;
    LR_TRY(g->allocate((size_t)max_batch * (size_t)std::max(g->beta, 1) * N));
    if (cP) LR_HIP(hipMalloc((void **)&g->d_pool, (size_t)g->chunk * ((size_t)g->beta * g->rows() + g->nQ) * N * sizeof(u64)));
    *out = g.release();
    return LR_OK;
    });
}

extern "C" int lr_keygen_destroy(lr_keygen *g) {
    return guarded([&]() -> int { return destroy_handle(g); });
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
