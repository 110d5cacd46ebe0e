// lr_setup.cpp -- C ABI: lr_setup, the collective key setup of dckks and dbfv for a batch of parties on the device: CKGProtocol.GenShare
// (dbfv/publickey_gen.go:54-57), the three rounds and the finalize of RKGProtocol (dbfv/relinkey_gen.go:215-355), the two rounds and the
// finalize of RKGProtocolNaive (dbfv/relinkey_gen_naive.go:59-200), RTGProtocol.genShare and Finalize (dbfv/rotkey_gen.go:139-215), and
// every Aggregate* as one n-ary fold over all of Q||P.  The dckks twins compute the same lines but for relinkey_gen_naive.go:73-75 (below).
// The randomness arrives in the compact form of the encryptors; crs and crp are the caller's polys.  Kernels: lr_setup.hip, the expansion
// of lr_ckks_encrypt.hip and the fold of lr_collective.hip.
// The host sanitizer build (tests/host_stub_build.py) compiles this unit with every other; the launchers of lr_setup.hip have their
// stand-in in tests/cpp/hipstub/stub_setup.cpp.
#include "lr_qp_handle.hpp"

// what the four New*Protocol constructors build: polypool / tmpPoly over Q||P, and here the pool of the transformed samples of one pass
struct lr_setup : lr_host::QpHandle {
    int alpha = 0, beta = 0, chunk = 0;       // chunk: parties per pass, min(max_batch, kSetupPartiesPerLaunch)
    u64 *d_pool = nullptr;                    // chunk * 3 beta sample polys over Q||P (two noises and a ternary per digit), then one tmp poly
    u64 *d_fold = nullptr;                    // the running sum of lr_setup_aggregate: max(2 beta, 1) polys over Q||P
    ~lr_setup() {
        for (void *p : {(void *)d_pool, (void *)d_fold})
            if (p) (void)hipFree(p);
    }
};

namespace lr_host {
namespace {

typedef const unsigned char *bytes_t;

int check_n(const lr_setup *s, int n, const char *what) {
    if (n < 1) return s->refuse(LR_ERR_SHAPE, std::string(what) + " must be at least 1");
    if (n > s->max_batch) return s->refuse(LR_ERR_SHAPE, std::string(what) + " exceeds the handle's max_batch");
    return LR_OK;
}

int need_p(const lr_setup *s) {
    return s->cP ? LR_OK : s->refuse(LR_ERR_ARG, "modulus P is empty: only CKG and its aggregation work over Q");
}

// a share of `members` polys, or a poly the call reads whole: its context, its limbs, its batch
int check_members(const lr_setup *s, const lr_poly *p, int members, const char *what) {
    if (p->ctx != s->cQ) return s->refuse(LR_ERR_ARG, std::string(what) + " belongs to another context");
    if (p->N != s->cQ->h.N || p->limbs < s->rows()) return s->refuse(LR_ERR_SHAPE, std::string(what) + " has too few limbs");
    if (p->batch != members) return s->refuse(LR_ERR_SHAPE, std::string(what) + "'s batch is not " + (members == s->beta ? "beta" : "2 beta"));
    return LR_OK;
}

// the n outputs of a share call, of `members` polys each, against the inputs and each other
int check_shares(const lr_setup *s, lr_poly *const *shares, int n, int members, std::initializer_list<const lr_poly *> ins) {
    for (int k = 0; k < n; ++k) {
        if (!shares[k]) return fail(LR_ERR_ARG, "null argument");
        LR_TRY(check_members(s, shares[k], members, "a share"));
        for (const lr_poly *in : ins)
            if (overlap(shares[k], in)) return s->refuse(LR_ERR_ARG, "an output shares memory with an input");
        for (int j = 0; j < k; ++j)
            if (overlap(shares[k], shares[j])) return s->refuse(LR_ERR_ARG, "two outputs share memory");
    }
    return LR_OK;
}

int begin(lr_setup *s) {
    if (s->cP) LR_TRY(same_stream(s->cQ, s->cP));
    LR_HIP(hipSetDevice(s->device));
    return LR_OK;
}

// noise polys, then ternary polys (either may be 0 items), one behind the other from `out` on, and Context.NTT over all of them
int sample_ntt(lr_setup *s, bytes_t eb, int noise_items, bytes_t coeff_bits, bytes_t sign_bits, int ternary_items, u64 *out, long long stride) {
    if (noise_items) LR_TRY(expand_qp(s, 0, s->rows(), 0, nullptr, nullptr, 1, eb, nullptr, out, stride, 0, noise_items));
    if (ternary_items)
        LR_TRY(expand_qp(s, 0, s->rows(), 1, coeff_bits, sign_bits, 0, nullptr, nullptr, out + noise_items * stride, stride, 0, ternary_items));
    return ntt_qp(s, s->cP != nullptr, false, s->nQ, noise_items + ternary_items, out, stride, out, stride);
}

// digit i owns rows [d0, d1) of Q: the loop of dbfv/relinkey_gen.go:235-250 with its break
void digit_rows(const lr_setup *s, int i, int *d0, int *d1) {
    *d0 = i * s->alpha;
    *d1 = std::min((i + 1) * s->alpha, s->nQ);
}

// one Context call of contextQP on one poly
int qp(lr_setup *s, int op, const u64 *a, const u64 *b, u64 *out) { return ewise_qp(s, true, op, 1, a, 0, b, 0, out, 0); }

u64 *tmp_poly(const lr_setup *s) { return s->d_pool + (long long)s->chunk * 3 * s->beta * s->rows() * (long long)s->cQ->h.N; }

// polypool = InvMForm(MulScalarBigint(sk, P)) over the rows of Q (dbfv/relinkey_gen.go:223-227; with a Galois element, rotkey_gen.go:143-146)
int times_p_call_by_call(lr_setup *s, const u64 *sk, u64 gen, u64 *tmp) {
    lr_context *cQ = s->cQ;
    if (gen != 1) LR_TRY(run_permute_ntt(cQ, s->nQ, 1, sk, 0, tmp, 0, gen));
    LR_TRY(run_ewise(cQ, LR_MUL_SCALAR_LIMBS, s->nQ, 1, gen != 1 ? tmp : sk, 0, nullptr, 0, tmp, 0, &s->pmont));
    return run_ewise(cQ, LR_INV_MFORM, s->nQ, 1, tmp, 0, nullptr, 0, tmp, 0, nullptr);
}

int add_digit_rows(lr_setup *s, int i, const u64 *tmp, u64 *x) {
    int d0, d1;
    digit_rows(s, i, &d0, &d1);
    const long long off = (long long)d0 * (long long)s->cQ->h.N;
    return run_ewise(s->cQ, LR_ADD, d1 - d0, 1, x + off, 0, tmp + off, 0, x + off, 0, nullptr, d0);
}

SetupShareLaunch share_launch(const lr_setup *s) {
    SetupShareLaunch L;
    std::memset(&L, 0, sizeof L);
    L.e = s->d_pool;
    L.e_stride = L.t_stride = (long long)s->rows() * (long long)s->cQ->h.N;
    L.n = (int)s->cQ->h.N;
    L.logn = (int)s->cQ->h.logN;
    L.nQ = s->nQ;
    L.alpha = s->alpha;
    L.beta = s->beta;
    L.pmont = s->pmont;
    L.lp = s->d_lp;
    return L;
}

// CKGProtocol.GenShare (dbfv/publickey_gen.go:54-57, dckks/publickey_gen.go:39-42)
int ckg_share(lr_setup *s, const lr_poly *sk, const lr_poly *crs, bytes_t eb, int batch, lr_poly *share, bool on_device) {
    if (!s || !sk || !crs || !eb || !share) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_n(s, batch, "batch"));
    LR_TRY(s->check_poly(sk, s->rows(), batch, true, "the secret key"));
    LR_TRY(s->check_poly(crs, s->rows(), batch, true, "crs"));
    LR_TRY(s->check_poly(share, s->rows(), batch, false, "the share"));
    if (overlap(share, sk) || overlap(share, crs)) return s->refuse(LR_ERR_ARG, "an output shares memory with an input");
    LR_TRY(begin(s));
    if (!on_device) LR_TRY(s->stage_random(&eb, (size_t)batch * (size_t)s->cQ->h.N));
    LR_TRY(sample_ntt(s, eb, batch, nullptr, nullptr, 0, share->d, share->stride()));                                     // :55 SampleNTT
    const long long ss = key_stride(sk, batch), cs = key_stride(crs, batch);
    if (s->call_by_call) return ewise_qp(s, s->cP != nullptr, LR_MUL_MONT_AND_SUB, batch, sk->d, ss, crs->d, cs, share->d, share->stride());   // :56
    SetupCkgLaunch L;
    L.sk = sk->d; L.sk_stride = ss;
    L.crs = crs->d; L.crs_stride = cs;
    L.share = share->d; L.share_stride = share->stride();
    L.n = (int)s->cQ->h.N;
    L.lp = s->d_lp;
    LR_HIP(launch_setup_ckg(L, s->rows(), batch, s->cQ->stream));
    return LR_OK;
}

struct ShareCall {
    int kind;
    const lr_poly *sk, *u, *crp, *in, *pk0, *pk1;
    bytes_t e, coeff_bits, sign_bits;
    const u64 *gens;
    int quirk;
};

// the call-by-call shape of one party's (RTG: one Galois element's) share: one launch per Context call of the reference, the samplers'
// writes standing as copies out of the pool
int share_call_by_call(lr_setup *s, const ShareCall &c, int k, int z0, int per, lr_poly *share) {
    const int beta = s->beta;
    const long long stride = (long long)s->rows() * (long long)s->cQ->h.N;
    u64 *tmp = tmp_poly(s);
    const u64 *sk = c.sk->d + (c.kind == kSetupRtg ? 0 : k * key_stride(c.sk, 2));
    const u64 *u = c.u ? c.u->d + k * key_stride(c.u, 2) : nullptr;
    const auto E = [&](int i, int comp) { return s->d_pool + (long long)((z0 + i) * per + comp) * stride; };
    const auto M = [&](const lr_poly *p, int m) { return p->d + (long long)m * p->stride(); };
    if (c.kind == kSetupRkg1 || c.kind == kSetupNaive1) LR_TRY(times_p_call_by_call(s, sk, 1, tmp));
    if (c.kind == kSetupRtg) LR_TRY(times_p_call_by_call(s, sk, c.gens[k], tmp));      // (the element 1 permutes nothing)
    if (c.kind == kSetupRkg3) LR_TRY(qp(s, LR_SUB, u, sk, tmp));                                                           // relinkey_gen.go:325
    for (int i = 0; i < beta; ++i) {
        switch (c.kind) {
            case kSetupRkg1:
                LR_TRY(qp(s, LR_COPY, E(i, 0), nullptr, M(share, i)));                                                    // :232
                LR_TRY(add_digit_rows(s, i, tmp, M(share, i)));                                                           // :235-250
                LR_TRY(qp(s, LR_MUL_MONT_AND_SUB, u, M(c.crp, i), M(share, i)));                                          // :253
                break;
            case kSetupRkg2:
                LR_TRY(qp(s, LR_MUL_MONT, M(c.in, i), sk, M(share, 2 * i)));                                              // :286
                LR_TRY(qp(s, LR_ADD, M(share, 2 * i), E(i, 0), M(share, 2 * i)));                                         // :289-290
                LR_TRY(qp(s, LR_COPY, E(i, 1), nullptr, M(share, 2 * i + 1)));                                            // :294
                LR_TRY(qp(s, LR_MUL_MONT_AND_ADD, sk, M(c.crp, i), M(share, 2 * i + 1)));                                 // :296
                break;
            case kSetupRkg3:
                LR_TRY(qp(s, LR_COPY, E(i, 0), nullptr, M(share, i)));                                                    // :330
                LR_TRY(qp(s, LR_MUL_MONT_AND_ADD, tmp, M(c.in, 2 * i + 1), M(share, i)));                                 // :331
                break;
            case kSetupNaive1:
                if (c.quirk) {      // dckks/relinkey_gen_naive.go:73-75: both draws into [i][0], [i][1] as allocated
                    LR_TRY(qp(s, LR_COPY, E(i, 0), nullptr, M(share, 2 * i)));
                    LR_TRY(qp(s, LR_COPY, E(i, 1), nullptr, M(share, 2 * i)));
                    LR_HIP(hipMemsetAsync(M(share, 2 * i + 1), 0, (size_t)stride * sizeof(u64), s->cQ->stream));
                } else {
                    LR_TRY(qp(s, LR_COPY, E(i, 0), nullptr, M(share, 2 * i)));                                            // relinkey_gen_naive.go:74
                    LR_TRY(qp(s, LR_COPY, E(i, 1), nullptr, M(share, 2 * i + 1)));                                        // :76
                }
                LR_TRY(add_digit_rows(s, i, tmp, M(share, 2 * i)));                                                       // :80-97
                break;
            case kSetupNaive2:
                LR_TRY(qp(s, LR_MUL_MONT, M(c.in, 2 * i), sk, M(share, 2 * i)));                                          // :143
                LR_TRY(qp(s, LR_MUL_MONT, M(c.in, 2 * i + 1), sk, M(share, 2 * i + 1)));                                  // :144
                break;
            default:
                LR_TRY(qp(s, LR_COPY, E(i, 0), nullptr, M(share, i)));                                                    // rotkey_gen.go:153
                LR_TRY(add_digit_rows(s, i, tmp, M(share, i)));                                                           // :159-175
                LR_TRY(qp(s, LR_MUL_MONT_AND_SUB, M(c.crp, i), sk, M(share, i)));                                         // :178
                LR_TRY(qp(s, LR_MFORM, M(share, i), nullptr, M(share, i)));                                               // :179
        }
    }
    return LR_OK;
}

// the lines of the naive rounds that read the transformed ternary `t` of digit i (relinkey_gen_naive.go:100-107, :147-161)
int naive_tail_call_by_call(lr_setup *s, const ShareCall &c, int i, const u64 *t, const u64 *e0, const u64 *e1, lr_poly *share) {
    u64 *o0 = share->d + (long long)(2 * i) * share->stride(), *o1 = share->d + (long long)(2 * i + 1) * share->stride();
    LR_TRY(qp(s, LR_MUL_MONT_AND_ADD, c.pk0->d, t, o0));
    LR_TRY(qp(s, LR_MUL_MONT_AND_ADD, c.pk1->d, t, o1));
    if (c.kind == kSetupNaive1) return LR_OK;
    LR_TRY(qp(s, LR_ADD, o0, e0, o0));
    return qp(s, LR_ADD, o1, e1, o1);
}

// every share call behind its checks: `per` noise polys and `ternary` (0 or 1) ternary polys per party and digit, passes of `chunk` parties
int run_shares(lr_setup *s, const ShareCall &c, int n, int per, int ternary, lr_poly *const *shares, bool on_device) {
    LR_TRY(begin(s));
    const long long N = (long long)s->cQ->h.N, stride = (long long)s->rows() * N;
    const int beta = s->beta;
    bytes_t eb = c.e, cb = c.coeff_bits, sb = c.sign_bits;
    if (!on_device) {
        const size_t noise = (size_t)n * beta * per * (size_t)N, plane = ternary ? (size_t)n * beta * (size_t)(N >> 3) : 0;
        bytes_t src[3] = {eb, cb, sb}, dev[3];
        const size_t bytes[3] = {noise, plane, plane};
        LR_TRY(s->stage_random(src, bytes, ternary ? 3 : 1, dev));
        eb = dev[0];
        if (ternary) cb = dev[1], sb = dev[2];
    }
    const u64 mask2 = 2 * (u64)N - 1;
    for (int first = 0; first < n; first += s->chunk) {
        const int parties = std::min(s->chunk, n - first), items = parties * beta;
        u64 *t = s->d_pool + (long long)items * per * stride;
        LR_TRY(sample_ntt(s, eb + (long long)first * beta * per * N, items * per, ternary ? cb + (long long)first * beta * (N >> 3) : nullptr,
                          ternary ? sb + (long long)first * beta * (N >> 3) : nullptr, ternary ? items : 0, s->d_pool, stride));
        if (s->call_by_call) {
            for (int k = 0; k < parties; ++k) {
                LR_TRY(share_call_by_call(s, c, first + k, k * beta, per, shares[first + k]));
                for (int i = 0; ternary && i < beta; ++i) {
                    const long long z = k * beta + i;
                    LR_TRY(naive_tail_call_by_call(s, c, i, t + z * stride, s->d_pool + 2 * z * stride, s->d_pool + (2 * z + 1) * stride, shares[first + k]));
                }
            }
            continue;
        }
        SetupShareLaunch L = share_launch(s);
        L.t = t;
        L.sk = c.sk->d + (c.kind == kSetupRtg ? 0 : first * key_stride(c.sk, n));
        L.sk_stride = c.kind == kSetupRtg ? 0 : key_stride(c.sk, n);
        if (c.u) L.u = c.u->d + first * key_stride(c.u, n), L.u_stride = key_stride(c.u, n);
        if (c.crp) L.crp = c.crp->d, L.crp_stride = c.crp->stride();
        if (c.in) L.in = c.in->d, L.in_stride = c.in->stride();
        if (c.pk0) L.pk0 = c.pk0->d, L.pk1 = c.pk1->d;
        L.quirk = c.quirk;
        for (int k = 0; k < parties; ++k) {
            L.out[k] = KeygenKeyRef{shares[first + k]->d, shares[first + k]->stride()};
            L.gen[k] = c.gens ? (u32)(c.gens[first + k] & mask2) : 1u;
        }
        LR_HIP(launch_setup_share(c.kind, L, s->rows(), parties, s->cQ->stream));
    }
    return LR_OK;
}

// a key of the call: one per party, or one for all
int check_key(const lr_setup *s, const lr_poly *p, int n, const char *what) { return s->check_poly(p, s->rows(), n, true, what); }

int rkg_round1(lr_setup *s, const lr_poly *u, const lr_poly *sk, const lr_poly *crp, bytes_t e, int n, lr_poly *const *shares, bool on_device) {
    if (!s || !u || !sk || !crp || !e || !shares) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(need_p(s));
    LR_TRY(check_n(s, n, "n_parties"));
    LR_TRY(check_key(s, u, n, "the ephemeral key"));
    LR_TRY(check_key(s, sk, n, "the secret key"));
    LR_TRY(check_members(s, crp, s->beta, "crp"));
    LR_TRY(check_shares(s, shares, n, s->beta, {u, sk, crp}));
    ShareCall c{kSetupRkg1, sk, u, crp, nullptr, nullptr, nullptr, e, nullptr, nullptr, nullptr, 0};
    return run_shares(s, c, n, 1, 0, shares, on_device);
}

int rkg_round2(lr_setup *s, const lr_poly *round1, const lr_poly *sk, const lr_poly *crp, bytes_t e, int n, lr_poly *const *shares, bool on_device) {
    if (!s || !round1 || !sk || !crp || !e || !shares) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(need_p(s));
    LR_TRY(check_n(s, n, "n_parties"));
    LR_TRY(check_members(s, round1, s->beta, "the round-one aggregate"));
    LR_TRY(check_key(s, sk, n, "the secret key"));
    LR_TRY(check_members(s, crp, s->beta, "crp"));
    LR_TRY(check_shares(s, shares, n, 2 * s->beta, {round1, sk, crp}));
    ShareCall c{kSetupRkg2, sk, nullptr, crp, round1, nullptr, nullptr, e, nullptr, nullptr, nullptr, 0};
    return run_shares(s, c, n, 2, 0, shares, on_device);
}

int rkg_round3(lr_setup *s, const lr_poly *round2, const lr_poly *u, const lr_poly *sk, bytes_t e, int n, lr_poly *const *shares, bool on_device) {
    if (!s || !round2 || !u || !sk || !e || !shares) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(need_p(s));
    LR_TRY(check_n(s, n, "n_parties"));
    LR_TRY(check_members(s, round2, 2 * s->beta, "the round-two aggregate"));
    LR_TRY(check_key(s, u, n, "the ephemeral key"));
    LR_TRY(check_key(s, sk, n, "the secret key"));
    LR_TRY(check_shares(s, shares, n, s->beta, {round2, u, sk}));
    ShareCall c{kSetupRkg3, sk, u, nullptr, round2, nullptr, nullptr, e, nullptr, nullptr, nullptr, 0};
    return run_shares(s, c, n, 1, 0, shares, on_device);
}

int naive_round(lr_setup *s, int kind, int scheme, const lr_poly *round1, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1, bytes_t e,
                bytes_t coeff_bits, bytes_t sign_bits, int n, lr_poly *const *shares, bool on_device) {
    if (!s || !sk || !pk0 || !pk1 || !e || !coeff_bits || !sign_bits || !shares || (kind == kSetupNaive2 && !round1)) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(need_p(s));
    if (scheme != LR_SETUP_BFV && scheme != LR_SETUP_CKKS) return s->refuse(LR_ERR_ARG, "scheme is neither LR_SETUP_BFV nor LR_SETUP_CKKS");
    LR_TRY(check_n(s, n, "n_parties"));
    if (round1) LR_TRY(check_members(s, round1, 2 * s->beta, "the round-one aggregate"));
    LR_TRY(check_key(s, sk, n, "the secret key"));
    LR_TRY(s->check_poly(pk0, s->rows(), 1, false, "the public key"));
    LR_TRY(s->check_poly(pk1, s->rows(), 1, false, "the public key"));
    if (round1) LR_TRY(check_shares(s, shares, n, 2 * s->beta, {round1, sk, pk0, pk1}));
    else LR_TRY(check_shares(s, shares, n, 2 * s->beta, {sk, pk0, pk1}));
    ShareCall c{kind, sk, nullptr, nullptr, round1, pk0, pk1, e, coeff_bits, sign_bits, nullptr, kind == kSetupNaive1 && scheme == LR_SETUP_CKKS};
    return run_shares(s, c, n, 2, 1, shares, on_device);
}

int rtg_share(lr_setup *s, const lr_poly *sk, const u64 *gens, int n_keys, const lr_poly *crp, bytes_t e, lr_poly *const *shares, bool on_device) {
    if (!s || !sk || !gens || !crp || !e || !shares) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(need_p(s));
    LR_TRY(check_n(s, n_keys, "n_keys"));
    LR_TRY(s->check_poly(sk, s->rows(), 1, false, "the secret key"));
    LR_TRY(check_members(s, crp, s->beta, "crp"));
    LR_TRY(check_shares(s, shares, n_keys, s->beta, {sk, crp}));
    for (int k = 0; k < n_keys; ++k)
        if (!(gens[k] & 1)) return s->refuse(LR_ERR_ARG, "a Galois element is even");
    std::vector<u64> reduced(gens, gens + n_keys);     // modulo 2 N: what PermuteNTTIndex reads of it
    for (u64 &g : reduced) g &= 2 * (u64)s->cQ->h.N - 1;
    ShareCall c{kSetupRtg, sk, nullptr, crp, nullptr, nullptr, nullptr, e, nullptr, nullptr, reduced.data(), 0};
    return run_shares(s, c, n_keys, 1, 0, shares, on_device);
}

// GenRelinearizationKey of both RKG protocols (dbfv/relinkey_gen.go:343-354, relinkey_gen_naive.go:187-200; round3 == nullptr: naive) and
// RTGProtocol.Finalize (dbfv/rotkey_gen.go:205-214; pairs == nullptr)
int finalize(lr_setup *s, const lr_poly *pairs, const lr_poly *polys, const lr_poly *crp, lr_poly *key, bool naive) {
    if (!s || !key || (!pairs && (!polys || !crp)) || (pairs && !naive && !polys)) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(need_p(s));
    const int beta = s->beta;
    if (pairs) LR_TRY(check_members(s, pairs, 2 * beta, "the round-two aggregate"));
    if (polys) LR_TRY(check_members(s, polys, beta, pairs ? "the round-three aggregate" : "the share"));
    if (crp) LR_TRY(check_members(s, crp, beta, "crp"));
    LR_TRY(check_members(s, key, 2 * beta, "the key"));
    if (pairs && overlap(key, pairs) && !same_poly(key, pairs)) return s->refuse(LR_ERR_ARG, "the key overlaps the round-two aggregate without being it");
    if ((polys && overlap(key, polys)) || (crp && overlap(key, crp))) return s->refuse(LR_ERR_ARG, "an output shares memory with an input");
    LR_TRY(begin(s));
    const auto M = [](const lr_poly *p, int m) { return p->d + (long long)m * p->stride(); };
    if (s->call_by_call) {
        for (int i = 0; i < beta; ++i) {
            if (pairs) {
                if (polys) LR_TRY(qp(s, LR_ADD, M(pairs, 2 * i), M(polys, i), M(key, 2 * i)));                            // relinkey_gen.go:348
                else if (!same_poly(key, pairs)) LR_TRY(qp(s, LR_COPY, M(pairs, 2 * i), nullptr, M(key, 2 * i)));         // relinkey_gen_naive.go:194
                if (!same_poly(key, pairs)) LR_TRY(qp(s, LR_COPY, M(pairs, 2 * i + 1), nullptr, M(key, 2 * i + 1)));      // :349
                LR_TRY(qp(s, LR_MFORM, M(key, 2 * i), nullptr, M(key, 2 * i)));                                           // :351
                LR_TRY(qp(s, LR_MFORM, M(key, 2 * i + 1), nullptr, M(key, 2 * i + 1)));                                   // :352
            } else {
                LR_TRY(qp(s, LR_COPY, M(polys, i), nullptr, M(key, 2 * i)));                                              // rotkey_gen.go:210
                LR_TRY(qp(s, LR_MFORM, M(crp, i), nullptr, M(key, 2 * i + 1)));                                           // :211
            }
        }
        return LR_OK;
    }
    SetupKeyLaunch L;
    std::memset(&L, 0, sizeof L);
    if (pairs) L.pairs = pairs->d, L.pairs_stride = pairs->stride();
    if (polys) L.polys = polys->d, L.polys_stride = polys->stride();
    if (crp) L.crp = crp->d, L.crp_stride = crp->stride();
    L.key = key->d;
    L.key_stride = key->stride();
    L.n = (int)s->cQ->h.N;
    L.lp = s->d_lp;
    LR_HIP(launch_setup_key(L, s->rows(), beta, s->cQ->stream));
    return LR_OK;
}

// every Aggregate* of the four protocols over all of Q||P: polys of batch 1 (CKG), beta or 2 beta
int aggregate(lr_setup *s, const lr_poly *const *shares, int n_shares, lr_poly *out) {
    if (!s || !shares || !out) return fail(LR_ERR_ARG, "null argument");
    if (n_shares < 1) return s->refuse(LR_ERR_SHAPE, "n_shares must be at least 1");
    if (out->batch != 1 && !(s->cP && (out->batch == s->beta || out->batch == 2 * s->beta)))
        return s->refuse(LR_ERR_SHAPE, "the output's batch is not 1, beta or 2 beta");
    if (s->cP) LR_TRY(same_stream(s->cQ, s->cP));
    return fold_rows(s, s->d_fold, s->nQ, s->cP != nullptr, nullptr, shares, n_shares, out);
}

}  // namespace
}  // namespace lr_host

extern "C" int lr_setup_create(lr_context *cQ, lr_context *cP, int max_batch, lr_setup **out) {
    return lr_setup_create_ex(cQ, cP, max_batch, nullptr, out);
}

extern "C" int lr_setup_create_ex(lr_context *cQ, lr_context *cP, int max_batch, const lr_options *options, lr_setup **out) {
    return guarded([&]() -> int {
    if (!cQ || !out) return fail(LR_ERR_ARG, "null argument");
    *out = nullptr;
    const char *name = "collective setup";
    Options parsed;
    LR_TRY(check_create(name, cQ, max_batch, options, &parsed));
    if (cQ->h.logN > 30) return fail(LR_ERR_UNSUPPORTED, "collective setup: ring degree");
    LR_TRY(check_pair(cQ, cP));
    std::unique_ptr<lr_setup> s(new lr_setup());
    LR_TRY(s->init(name, cQ, cP, max_batch, parsed));
    s->chunk = std::min(max_batch, kSetupPartiesPerLaunch);
    s->alpha = s->nP;                                                // params.Alpha() = |P|, Beta() = ceil(|Q| / |P|)
    s->beta = cP ? (s->nQ + s->nP - 1) / s->nP : 0;
    LR_HIP(hipSetDevice(cQ->device));
    const size_t N = (size_t)cQ->h.N, poly = (size_t)s->rows() * N * sizeof(u64);
    // the largest host-form call: the naive rounds' two noise polys and two bit planes per party and digit
    LR_TRY(s->allocate((size_t)max_batch * (size_t)std::max(s->beta, 1) * (2 * N + 2 * (N >> 3))));
    if (cP) LR_HIP(hipMalloc((void **)&s->d_pool, ((size_t)s->chunk * 3 * s->beta + 1) * poly));
    LR_HIP(hipMalloc((void **)&s->d_fold, (size_t)std::max(2 * s->beta, 1) * poly));
    *out = s.release();
    return LR_OK;
    });
}

extern "C" int lr_setup_destroy(lr_setup *s) {
    return guarded([&]() -> int { return destroy_handle(s); });
}

typedef const unsigned char *bytes_t;

extern "C" int lr_setup_ckg_share(lr_setup *s, const lr_poly *sk, const lr_poly *crs, const uint8_t *e, int batch, lr_poly *share_out) {
    return guarded([&]() -> int { return ckg_share(s, sk, crs, e, batch, share_out, false); });
}
extern "C" int lr_setup_ckg_share_device(lr_setup *s, const lr_poly *sk, const lr_poly *crs, const void *e, int batch, lr_poly *share_out) {
    return guarded([&]() -> int { return ckg_share(s, sk, crs, (bytes_t)e, batch, share_out, true); });
}
extern "C" int lr_setup_rkg_round1(lr_setup *s, const lr_poly *u, const lr_poly *sk, const lr_poly *crp, const uint8_t *e, int n_parties,
                                   lr_poly *const *shares) {
    return guarded([&]() -> int { return rkg_round1(s, u, sk, crp, e, n_parties, shares, false); });
}
extern "C" int lr_setup_rkg_round1_device(lr_setup *s, const lr_poly *u, const lr_poly *sk, const lr_poly *crp, const void *e, int n_parties,
                                          lr_poly *const *shares) {
    return guarded([&]() -> int { return rkg_round1(s, u, sk, crp, (bytes_t)e, n_parties, shares, true); });
}
extern "C" int lr_setup_rkg_round2(lr_setup *s, const lr_poly *round1, const lr_poly *sk, const lr_poly *crp, const uint8_t *e, int n_parties,
                                   lr_poly *const *shares) {
    return guarded([&]() -> int { return rkg_round2(s, round1, sk, crp, e, n_parties, shares, false); });
}
extern "C" int lr_setup_rkg_round2_device(lr_setup *s, const lr_poly *round1, const lr_poly *sk, const lr_poly *crp, const void *e, int n_parties,
                                          lr_poly *const *shares) {
    return guarded([&]() -> int { return rkg_round2(s, round1, sk, crp, (bytes_t)e, n_parties, shares, true); });
}
extern "C" int lr_setup_rkg_round3(lr_setup *s, const lr_poly *round2, const lr_poly *u, const lr_poly *sk, const uint8_t *e, int n_parties,
                                   lr_poly *const *shares) {
    return guarded([&]() -> int { return rkg_round3(s, round2, u, sk, e, n_parties, shares, false); });
}
extern "C" int lr_setup_rkg_round3_device(lr_setup *s, const lr_poly *round2, const lr_poly *u, const lr_poly *sk, const void *e, int n_parties,
                                          lr_poly *const *shares) {
    return guarded([&]() -> int { return rkg_round3(s, round2, u, sk, (bytes_t)e, n_parties, shares, true); });
}
extern "C" int lr_setup_rkg_key(lr_setup *s, const lr_poly *round2, const lr_poly *round3, lr_poly *evk_out) {
    return guarded([&]() -> int {
        if (!round2 || !round3) return fail(LR_ERR_ARG, "null argument");
        return finalize(s, round2, round3, nullptr, evk_out, false);
    });
}
extern "C" int lr_setup_rkg_naive_round1(lr_setup *s, int scheme, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1, const uint8_t *e,
                                         const uint8_t *u_coeff_bits, const uint8_t *u_sign_bits, int n_parties, lr_poly *const *shares) {
    return guarded([&]() -> int { return naive_round(s, kSetupNaive1, scheme, nullptr, sk, pk0, pk1, e, u_coeff_bits, u_sign_bits, n_parties, shares, false); });
}
extern "C" int lr_setup_rkg_naive_round1_device(lr_setup *s, int scheme, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1, const void *e,
                                                const void *u_coeff_bits, const void *u_sign_bits, int n_parties, lr_poly *const *shares) {
    return guarded([&]() -> int {
        return naive_round(s, kSetupNaive1, scheme, nullptr, sk, pk0, pk1, (bytes_t)e, (bytes_t)u_coeff_bits, (bytes_t)u_sign_bits, n_parties, shares, true);
    });
}
extern "C" int lr_setup_rkg_naive_round2(lr_setup *s, const lr_poly *round1, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1,
                                         const uint8_t *v_coeff_bits, const uint8_t *v_sign_bits, const uint8_t *e, int n_parties,
                                         lr_poly *const *shares) {
    return guarded([&]() -> int {
        if (!round1) return fail(LR_ERR_ARG, "null argument");
        return naive_round(s, kSetupNaive2, LR_SETUP_BFV, round1, sk, pk0, pk1, e, v_coeff_bits, v_sign_bits, n_parties, shares, false);
    });
}
extern "C" int lr_setup_rkg_naive_round2_device(lr_setup *s, const lr_poly *round1, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1,
                                                const void *v_coeff_bits, const void *v_sign_bits, const void *e, int n_parties,
                                                lr_poly *const *shares) {
    return guarded([&]() -> int {
        if (!round1) return fail(LR_ERR_ARG, "null argument");
        return naive_round(s, kSetupNaive2, LR_SETUP_BFV, round1, sk, pk0, pk1, (bytes_t)e, (bytes_t)v_coeff_bits, (bytes_t)v_sign_bits, n_parties, shares,
                           true);
    });
}
extern "C" int lr_setup_rkg_naive_key(lr_setup *s, const lr_poly *round2, lr_poly *evk_out) {
    return guarded([&]() -> int {
        if (!round2) return fail(LR_ERR_ARG, "null argument");
        return finalize(s, round2, nullptr, nullptr, evk_out, true);
    });
}
extern "C" int lr_setup_rtg_share(lr_setup *s, const lr_poly *sk, const uint64_t *galois_elements, int n_keys, const lr_poly *crp, const uint8_t *e,
                                  lr_poly *const *shares) {
    return guarded([&]() -> int { return rtg_share(s, sk, galois_elements, n_keys, crp, e, shares, false); });
}
extern "C" int lr_setup_rtg_share_device(lr_setup *s, const lr_poly *sk, const uint64_t *galois_elements, int n_keys, const lr_poly *crp,
                                         const void *e, lr_poly *const *shares) {
    return guarded([&]() -> int { return rtg_share(s, sk, galois_elements, n_keys, crp, (bytes_t)e, shares, true); });
}
extern "C" int lr_setup_rtg_key(lr_setup *s, const lr_poly *share, const lr_poly *crp, lr_poly *rotkey_out) {
    return guarded([&]() -> int {
        if (!share || !crp) return fail(LR_ERR_ARG, "null argument");
        return finalize(s, nullptr, share, crp, rotkey_out, false);
    });
}
extern "C" int lr_setup_aggregate(lr_setup *s, const lr_poly *const *shares, int n_shares, lr_poly *out) {
    return guarded([&]() -> int { return aggregate(s, shares, n_shares, out); });
}
