// lr_collective.cpp -- C ABI: lr_collective, the per-ciphertext protocols of dckks and dbfv for a batch of ciphertexts on the device:
// CKSProtocol.GenShare (dckks/keyswitching.go:62-94, dbfv/keyswitching.go:74-109), PCKSProtocol.GenShare
// (dckks/public_keyswitching.go:63-93, dbfv/public_keyswitching.go:111-148) and AggregateShares / KeySwitch of all four as one n-ary fold.
// The randomness arrives in the compact form of the encryptors (lr_bfv_encryptor).  Kernels: lr_collective.hip, the expansions of
// lr_ckks_encrypt.hip and lr_bfv_encrypt.hip, launch_mul2 and launch_ckks_pk_fast where the lines are pkEncryptor.encrypt's.
// The unit's name keeps it out of the lr_abi_*.cpp set that the shared sanitizer build links against its fixed launch stubs: the launchers
// it calls have a stand-in of their own (tests/cpp/collective_stub.cpp).
#include "lr_host.hpp"

// what the four New*Protocol constructors build (dckks/keyswitching.go:28-49, dckks/public_keyswitching.go:28-49 and their dbfv twins),
// plus the staging of the host-randomness entry points
struct lr_collective {
    int device = 0;
    lr_context *cQ = nullptr, *cP = nullptr;
    lr_bext *bext = nullptr;                  // NewFastBasisExtender(contextQ, contextP), owned
    int nQ = 0, nP = 0, max_batch = 0;
    bool call_by_call = false;                // Options::no_epilogue: the reference's call-by-call shape
    LimbScalars one, minus_one;               // matrixTernaryMontgomery rows 1 and 2 (ring/ring_context.go:119-122) per limb of Q||P
    LimbScalars pmont;                        // MForm(P mod q_j) per limb of Q: MulScalarBigint's scalar (ring/ring.go:547)
    LimbParams *d_lp = nullptr;               // the limb constants of contextQP: contextQ's, then contextP's
    u64 *d_pool = nullptr;                    // tmp, share0tmp, share1tmp: three polys over Q||P for max_batch ciphertexts
    u64 *d_zero = nullptr;                    // one poly of zeros over Q||P: the plaintext operand of launch_ckks_pk_fast
    unsigned char *d_rand = nullptr;          // the host-randomness entry points' bytes on the device ...
    unsigned char *h_rand = nullptr;          // ... and pinned: max_batch * (N / 4 + 2 N)
    hipEvent_t staged = nullptr;              // the last copy out of h_rand: the next call waits for it before it refills the buffer
    ~lr_collective() {
        for (void *p : {(void *)d_lp, (void *)d_pool, (void *)d_zero, (void *)d_rand})
            if (p) (void)hipFree(p);
        if (h_rand) (void)hipHostFree(h_rand);
        if (staged) (void)hipEventDestroy(staged);
        if (bext) lr_bext_destroy(bext);
    }
};

namespace lr_host {
namespace {

long long key_stride(const lr_poly *p, int batch) { return p->batch == 1 && batch > 1 ? 0 : p->stride(); }

// a poly of the handle's contextQ with at least `limbs` limbs and the call's batch (or, where allowed, one poly for the whole batch)
int check_poly(const lr_collective *h, const lr_poly *p, int limbs, int batch, bool broadcast, const char *what) {
    if (p->ctx != h->cQ) return fail(LR_ERR_ARG, std::string("collective: ") + what + " belongs to another context");
    if (p->N != h->cQ->h.N || p->limbs < limbs) return fail(LR_ERR_SHAPE, std::string("collective: ") + what + " has too few limbs");
    if (p->batch != batch && !(broadcast && p->batch == 1)) return fail(LR_ERR_SHAPE, std::string("collective: batch differs from the batch of ") + what);
    return LR_OK;
}

// the words of two polys overlap: an output that is, or lies inside, an input
bool overlap(const lr_poly *a, const lr_poly *b) {
    const u64 *a1 = a->d + (long long)(a->batch - 1) * a->stride() + (long long)a->alloc_limbs * (long long)a->N;
    const u64 *b1 = b->d + (long long)(b->batch - 1) * b->stride() + (long long)b->alloc_limbs * (long long)b->N;
    return a->d < b1 && b->d < a1;
}

// the same words, poly for poly: what an element-wise pass may read and write at once
bool same_poly(const lr_poly *a, const lr_poly *b) { return a->d == b->d && a->batch == b->batch && (a->batch == 1 || a->stride() == b->stride()); }

int check_call(const lr_collective *h, int level, int batch) {
    if (level < 0 || level + 1 > h->nQ) return fail(LR_ERR_SHAPE, "collective: level out of range");
    if (batch < 1) return fail(LR_ERR_SHAPE, "collective: batch must be at least 1");
    if (batch > h->max_batch) return fail(LR_ERR_SHAPE, "collective: batch exceeds the handle's max_batch");
    return same_stream(h->cQ, h->cP);
}

int check_outputs(const lr_poly *const *outs, int n_outs, const lr_poly *const *ins, int n_ins) {
    for (int o = 0; o < n_outs; ++o) {
        for (int i = 0; i < n_ins; ++i)
            if (overlap(outs[o], ins[i])) return fail(LR_ERR_ARG, "collective: an output shares memory with an input");
        for (int j = 0; j < o; ++j)
            if (overlap(outs[o], outs[j])) return fail(LR_ERR_ARG, "collective: the two outputs share memory");
    }
    return LR_OK;
}

// the three pool polys of a call, back to back: [3][batch][|Q| + |P|][N]
struct Pools {
    u64 *p[3];
    long long stride, part;
};
Pools pools_of(const lr_collective *h, int batch) {
    const long long n = (long long)h->cQ->h.N, s = (long long)(h->nQ + h->nP) * n;
    return Pools{{h->d_pool, h->d_pool + batch * s, h->d_pool + 2 * batch * s}, s, batch * s};
}

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

LimbScalars from_row(const LimbScalars &v, int row0) {
    LimbScalars r;
    std::memset(&r, 0, sizeof r);
    for (int i = row0; i < kMaxLimbs; ++i) r.v[i - row0] = v.v[i];
    return r;
}

// one Context call of contextQP on rows inside the pools: the Q rows under contextQ, the P rows under contextP
int ewise_qp(lr_collective *h, int op, int batch, const u64 *a, long long a_stride, const u64 *b, long long b_stride, u64 *out,
             long long out_stride) {
    const long long offP = (long long)h->nQ * (long long)h->cQ->h.N;
    LR_TRY(run_ewise(h->cQ, op, h->nQ, batch, a, a_stride, b, b_stride, out, out_stride, nullptr));
    return run_ewise(h->cP, op, h->nP, batch, a + offP, a_stride, b ? b + offP : nullptr, b_stride, out + offP, out_stride, nullptr);
}

// Context.NTT / InvNTT in place on `items` pool polys: limbs 0 .. level under contextQ, the rows of P under contextP
int ntt_rows(lr_collective *h, bool inverse, int level, u64 *p, long long stride, int items) {
    LR_TRY(run_ntt(h->cQ, inverse, Rows{p, stride, 0, 1}, Rows{p, stride, 0, 1}, 0, 1, level + 1, items));
    return run_ntt(h->cP, inverse, Rows{p, stride, h->nQ, 1}, Rows{p, stride, h->nQ, 1}, 0, 1, h->nP, items);
}

// SampleTernaryMontgomery and / or KYSampler.Sample as the forward transform's operands (the q of (0, sign 0) written as 0) on the rows a
// call at `level` reads: `ternary` + `noises` parts of `batch` polys from `out` on, part_stride apart
int expand(lr_collective *h, int level, int ternary, const unsigned char *u_coeff, const unsigned char *u_sign, int noises,
           const unsigned char *e0, const unsigned char *e1, u64 *out, long long stride, long long part, int batch) {
    Span s[2];
    const int n_spans = spans_of(h, level, s);
    for (int k = 0; k < n_spans; ++k) {
        CkksExpandLaunch X;
        std::memset(&X, 0, sizeof X);
        X.coeff_bits = u_coeff;
        X.sign_bits = u_sign;
        X.e[0] = e0;
        X.e[1] = e1;
        X.out = out + (long long)s[k].row0 * (long long)h->cQ->h.N;
        X.out_stride = stride;
        X.part_stride = part;
        X.n = (int)h->cQ->h.N;
        X.ternary = ternary;
        X.noises = noises;
        X.one = from_row(h->one, s[k].row0);
        X.minus_one = from_row(h->minus_one, s[k].row0);
        X.lp = h->d_lp + s[k].row0;
        LR_HIP(launch_ckks_expand(X, s[k].count, batch, h->cQ->stream));
    }
    return LR_OK;
}

// KYSampler.Sample into a pool poly over all of Q||P (add = 0, the residue q_j of (0, sign 0) as the reference stores it), or
// SampleAndAdd / Sample + Context.Add on `comps` pool polys (add = 1) over rows 0 .. rows - 1
int noise(lr_collective *h, int add, int comps, const unsigned char *const *eb, u64 *const *x, long long stride, int rows, int batch) {
    NoiseLaunch L;
    std::memset(&L, 0, sizeof L);
    for (int k = 0; k < comps; ++k) {
        L.x[k] = add ? x[k] : nullptr;
        L.out[k] = x[k];
        L.x_stride[k] = L.out_stride[k] = stride;
        L.e[k] = eb[k];
    }
    L.n = (int)h->cQ->h.N;
    L.add = add;
    L.lp = h->d_lp;
    LR_HIP(launch_bfv_noise(L, comps, rows, batch, h->cQ->stream));
    return LR_OK;
}

// the caller's bytes through the pinned buffer to the device, pieces one behind the other; the caller's arrays are free on return
int stage_random(lr_collective *h, const unsigned char *const *src, const size_t *bytes, int pieces, const unsigned char **dev) {
    LR_HIP(hipEventSynchronize(h->staged));               // the copy of the call before has left the pinned buffer
    size_t off = 0;
    for (int i = 0; i < pieces; ++i) {
        std::memcpy(h->h_rand + off, src[i], bytes[i]);
        dev[i] = h->d_rand + off;
        off += bytes[i];
    }
    LR_HIP(hipMemcpyAsync(h->d_rand, h->h_rand, off, hipMemcpyHostToDevice, h->cQ->stream));
    LR_HIP(hipEventRecord(h->staged, h->cQ->stream));
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
    LR_TRY(check_poly(h, sk_in, h->nQ, batch, true, "the input secret key"));
    LR_TRY(check_poly(h, sk_out, h->nQ, batch, true, "the output secret key"));
    LR_TRY(check_poly(h, c1, level + 1, batch, false, "the ciphertext"));
    LR_TRY(check_poly(h, share, level + 1, batch, false, "the share"));
    const lr_poly *outs[1] = {share}, *ins[3] = {sk_in, sk_out, c1};
    return check_outputs(outs, 1, ins, 3);
}

// CKSProtocol.GenShare of dckks (dckks/keyswitching.go:62-94)
int ckks_cks_share(lr_collective *h, int level, const lr_poly *sk_in, const lr_poly *sk_out, const lr_poly *c1, const unsigned char *eb, int batch,
                   lr_poly *share, bool on_device) {
    if (!h || !sk_in || !sk_out || !c1 || !eb || !share) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_cks(h, level, sk_in, sk_out, c1, batch, share));
    LR_HIP(hipSetDevice(h->device));
    if (!on_device) {
        const unsigned char *src[1] = {eb}, *dev[1];
        const size_t bytes[1] = {(size_t)batch * (size_t)h->cQ->h.N};
        LR_TRY(stage_random(h, src, bytes, 1, dev));
        eb = dev[0];
    }
    lr_context *cQ = h->cQ;
    const Pools P = pools_of(h, batch);
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
    if (!on_device) {
        const unsigned char *src[1] = {eb}, *dev[1];
        const size_t bytes[1] = {(size_t)batch * (size_t)h->cQ->h.N};
        LR_TRY(stage_random(h, src, bytes, 1, dev));
        eb = dev[0];
    }
    lr_context *cQ = h->cQ;
    const Pools P = pools_of(h, batch);
    const Rows q0{P.p[0], P.stride, 0, 1}, q2{P.p[2], P.stride, 0, 1};
    LR_TRY(run_ntt(cQ, false, Rows{c1->d, c1->stride(), 0, 1}, q0, 0, 1, h->nQ, batch));                              // :88
    if (h->call_by_call) {
        LR_TRY(delta_product(h, level, P.p[0], P.stride, sk_in, sk_out, P, batch));                                   // :76, :89, :90
        LR_TRY(run_ntt(cQ, true, q2, q2, 0, 1, h->nQ, batch));                                                        // :92
        LR_TRY(noise(h, 0, 1, &eb, &P.p[0], P.stride, h->nQ + h->nP, batch));                                         // :94 Sample over Q||P
        LR_TRY(run_ewise(cQ, LR_ADD, h->nQ, batch, P.p[2], P.stride, P.p[0], P.stride, P.p[2], P.stride, nullptr));   // :95
        // :97-103: hP = the rows of P as they are, p_j of (0, sign 0) included
        return moddown_pq_core(h->bext, level, P.p[2], P.stride, Rows{P.p[0], P.stride, h->nQ, 1}, batch, share, false);   // :105
    }
    LR_HIP(launch_cks_share(share_launch(h, P.p[0], P.stride, sk_in, sk_out, nullptr, P.p[0], P.stride, batch), h->nQ, batch, cQ->stream));
    LR_TRY(run_ntt(cQ, true, q0, q0, 0, 1, h->nQ, batch));
    LR_TRY(noise(h, 1, 1, &eb, &P.p[0], P.stride, h->nQ, batch));                           // CRed(x + residue) on the rows of Q
    {   // the residue on the rows of P, p_j written as 0: no bit of the ModDown's output changes (tests/test_oracle_collective.py)
        CkksExpandLaunch X;
        std::memset(&X, 0, sizeof X);
        X.e[0] = eb;
        X.out = P.p[0] + (long long)h->nQ * (long long)cQ->h.N;
        X.out_stride = P.stride;
        X.n = (int)cQ->h.N;
        X.noises = 1;
        X.lp = h->d_lp + h->nQ;
        LR_HIP(launch_ckks_expand(X, h->nP, batch, cQ->stream));
    }
    return moddown_pq_core(h->bext, level, P.p[0], P.stride, Rows{P.p[0], P.stride, h->nQ, 1}, batch, share, false);
}

struct PcksRandom { const unsigned char *u_coeff, *u_sign, *e0, *e1; };

int check_pcks(const lr_collective *h, int level, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1, const lr_poly *c1, int batch,
               const lr_poly *o0, const lr_poly *o1) {
    LR_TRY(check_call(h, level, batch));
    LR_TRY(check_poly(h, sk, h->nQ, batch, true, "the secret key"));
    LR_TRY(check_poly(h, pk0, h->nQ + h->nP, batch, true, "the public key"));
    LR_TRY(check_poly(h, pk1, h->nQ + h->nP, batch, true, "the public key"));
    LR_TRY(check_poly(h, c1, level + 1, batch, false, "the ciphertext"));
    LR_TRY(check_poly(h, o0, level + 1, batch, false, "the share"));
    LR_TRY(check_poly(h, o1, level + 1, batch, false, "the share"));
    const lr_poly *outs[2] = {o0, o1}, *ins[4] = {sk, pk0, pk1, c1};
    return check_outputs(outs, 2, ins, 4);
}

int stage_pcks(lr_collective *h, PcksRandom *R, int batch) {
    const size_t N = (size_t)h->cQ->h.N, plane = (size_t)batch * (N >> 3), bytes_e = (size_t)batch * N;
    const unsigned char *src[4] = {R->u_coeff, R->u_sign, R->e0, R->e1}, *dev[4];
    const size_t bytes[4] = {plane, plane, bytes_e, bytes_e};
    LR_TRY(stage_random(h, src, bytes, 4, dev));
    *R = PcksRandom{dev[0], dev[1], dev[2], dev[3]};
    return LR_OK;
}

// SampleTernaryMontgomeryNTT over Q||P (dckks/public_keyswitching.go:68, dbfv :116) into P.p[2]
int ternary_ntt(lr_collective *h, const PcksRandom &R, const Pools &P, int batch) {
    TernaryLaunch T;
    T.coeff_bits = R.u_coeff;
    T.sign_bits = R.u_sign;
    T.out = P.p[2];
    T.out_stride = P.stride;
    T.n = (int)h->cQ->h.N;
    T.one = h->one;
    T.minus_one = h->minus_one;
    LR_HIP(launch_bfv_ternary(T, h->nQ + h->nP, batch, h->cQ->stream));
    return ntt_rows(h, false, h->nQ - 1, P.p[2], P.stride, batch);
}

// PCKSProtocol.GenShare of dckks (dckks/public_keyswitching.go:63-93)
int ckks_pcks_share(lr_collective *h, int level, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1, const lr_poly *c1, PcksRandom R, int batch,
                    lr_poly *o0, lr_poly *o1, bool on_device) {
    if (!h || !sk || !pk0 || !pk1 || !c1 || !R.u_coeff || !R.u_sign || !R.e0 || !R.e1 || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_pcks(h, level, sk, pk0, pk1, c1, batch, o0, o1));
    LR_HIP(hipSetDevice(h->device));
    if (!on_device) LR_TRY(stage_pcks(h, &R, batch));
    lr_context *cQ = h->cQ;
    const Pools P = pools_of(h, batch);
    const long long n = (long long)cQ->h.N;
    const int L1 = level + 1, top = h->nQ - 1;
    const lr_poly *pk[2] = {pk0, pk1};
    lr_poly *outs[2] = {o0, o1};
    if (h->call_by_call) {
        const unsigned char *eb[2] = {R.e0, R.e1};
        LR_TRY(ternary_ntt(h, R, P, batch));                                                                          // :68
        for (int k = 0; k < 2; ++k)                                                                                   // :71, :73
            LR_TRY(ewise_qp(h, LR_MUL_MONT, batch, P.p[2], P.stride, pk[k]->d, key_stride(pk[k], batch), P.p[k], P.stride));
        for (int k = 0; k < 2; ++k) {                                                                                 // :76-80
            LR_TRY(expand(h, top, 0, nullptr, nullptr, 1, eb[k], nullptr, P.p[2], P.stride, P.part, batch));
            LR_TRY(ntt_rows(h, false, top, P.p[2], P.stride, batch));
            LR_TRY(ewise_qp(h, LR_ADD, batch, P.p[k], P.stride, P.p[2], P.stride, P.p[k], P.stride));
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
int bfv_pcks_share(lr_collective *h, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1, const lr_poly *c1, PcksRandom R, int batch, lr_poly *o0,
                   lr_poly *o1, bool on_device) {
    if (!h || !sk || !pk0 || !pk1 || !c1 || !R.u_coeff || !R.u_sign || !R.e0 || !R.e1 || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    const int level = h->nQ - 1, rows = h->nQ + h->nP;
    LR_TRY(check_pcks(h, level, sk, pk0, pk1, c1, batch, o0, o1));
    LR_HIP(hipSetDevice(h->device));
    if (!on_device) LR_TRY(stage_pcks(h, &R, batch));
    lr_context *cQ = h->cQ;
    const Pools P = pools_of(h, batch);
    const lr_poly *pk[2] = {pk0, pk1};
    lr_poly *outs[2] = {o0, o1};
    const unsigned char *eb[2] = {R.e0, R.e1};
    LR_TRY(ternary_ntt(h, R, P, batch));                                                                              // :116
    if (h->call_by_call) {
        for (int k = 0; k < 2; ++k)                                                                                   // :119, :121
            LR_TRY(ewise_qp(h, LR_MUL_MONT, batch, P.p[2], P.stride, pk[k]->d, key_stride(pk[k], batch), P.p[k], P.stride));
        for (int k = 0; k < 2; ++k) LR_TRY(ntt_rows(h, true, level, P.p[k], P.stride, batch));                        // :123-124
        for (int k = 0; k < 2; ++k) {                                                                                 // :127, :129: the residues as a poly, then Context.Add
            LR_TRY(noise(h, 0, 1, &eb[k], &P.p[2], P.stride, rows, batch));
            LR_TRY(ewise_qp(h, LR_ADD, batch, P.p[k], P.stride, P.p[2], P.stride, P.p[k], P.stride));
        }
    } else {
        Mul2Launch M;                    // both products in one pass over u, all rows of Q||P in one launch
        M.a = P.p[2]; M.a_stride = P.stride;
        M.b0 = pk0->d; M.b0_stride = key_stride(pk0, batch);
        M.b1 = pk1->d; M.b1_stride = key_stride(pk1, batch);
        M.out0 = P.p[0]; M.out1 = P.p[1];
        M.out0_stride = M.out1_stride = P.stride;
        M.n = (int)cQ->h.N;
        M.lp = h->d_lp;
        LR_HIP(launch_mul2(M, rows, batch, cQ->stream));
        LR_TRY(ntt_rows(h, true, level, P.p[0], P.stride, 2 * batch));                      // the two pools are back to back
        LR_TRY(noise(h, 1, 2, eb, P.p, P.stride, rows, batch));
    }
    for (int k = 0; k < 2; ++k)                                                                                       // :132, :136
        LR_TRY(moddown_pq_core(h->bext, level, P.p[k], P.stride, Rows{P.p[k], P.stride, h->nQ, 1}, batch, outs[k], false));
    const Rows q2{P.p[2], P.stride, 0, 1};
    LR_TRY(run_ntt(cQ, false, Rows{c1->d, c1->stride(), 0, 1}, q2, 0, 1, h->nQ, batch));                              // :139
    LR_TRY(run_ewise(cQ, LR_MUL_MONT, h->nQ, batch, P.p[2], P.stride, sk->d, key_stride(sk, batch), P.p[2], P.stride, nullptr));   // :140
    LR_TRY(run_ntt(cQ, true, q2, q2, 0, 1, h->nQ, batch));                                                            // :141
    return run_ewise(cQ, LR_ADD, h->nQ, batch, o0->d, o0->stride(), P.p[2], P.stride, o0->d, o0->stride(), nullptr);  // :144
}

// AggregateShares over n_shares parties and KeySwitch's Add (dckks/keyswitching.go:99-108 and its three twins)
int aggregate(lr_collective *h, int level, const lr_poly *base, const lr_poly *const *shares, int n_shares, lr_poly *out) {
    if (!h || !shares || !out) return fail(LR_ERR_ARG, "null argument");
    if (n_shares < 1) return fail(LR_ERR_SHAPE, "collective: n_shares must be at least 1");
    const int batch = out->batch;
    LR_TRY(check_call(h, level, batch));
    LR_TRY(check_poly(h, out, level + 1, batch, false, "the output"));
    if (base) {
        LR_TRY(check_poly(h, base, level + 1, batch, false, "the base"));
        if (overlap(out, base) && !same_poly(out, base)) return fail(LR_ERR_ARG, "collective: the output overlaps the base without being it");
    }
    for (int k = 0; k < n_shares; ++k) {
        if (!shares[k]) return fail(LR_ERR_ARG, "null argument");
        LR_TRY(check_poly(h, shares[k], level + 1, batch, false, "a share"));
        if (overlap(out, shares[k]) && !same_poly(out, shares[k])) return fail(LR_ERR_ARG, "collective: the output overlaps a share without being it");
    }
    LR_HIP(hipSetDevice(h->device));
    lr_context *cQ = h->cQ;
    const Pools P = pools_of(h, batch);
    const int L1 = level + 1;
    if (h->call_by_call) {     // n_shares - 1 Context.Add calls, then KeySwitch's; the running sum lives in the pool: out may be base or a share
        const u64 *acc = shares[0]->d;
        long long acc_stride = shares[0]->stride();
        for (int k = 1; k < n_shares; ++k) {
            const bool last = k == n_shares - 1 && !base;
            u64 *dst = last ? out->d : P.p[0];
            const long long dst_stride = last ? out->stride() : P.stride;
            LR_TRY(run_ewise(cQ, LR_ADD, L1, batch, acc, acc_stride, shares[k]->d, shares[k]->stride(), dst, dst_stride, nullptr));
            acc = dst;
            acc_stride = dst_stride;
        }
        if (base) return run_ewise(cQ, LR_ADD, L1, batch, base->d, base->stride(), acc, acc_stride, out->d, out->stride(), nullptr);
        if (n_shares == 1) return run_ewise(cQ, LR_COPY, L1, batch, acc, acc_stride, nullptr, 0, out->d, out->stride(), nullptr);
        return LR_OK;
    }
    // kFoldSharesPerLaunch shares per pass; a further pass takes the running sum, in the pool, as its first term
    for (int first = 0; first < n_shares;) {
        FoldLaunch F;
        std::memset(&F, 0, sizeof F);
        int count = 0;
        if (first > 0) F.share[count++] = FoldShareRef{P.p[0], P.stride};
        while (count < kFoldSharesPerLaunch && first < n_shares) {
            F.share[count++] = FoldShareRef{shares[first]->d, shares[first]->stride()};
            ++first;
        }
        const bool last = first == n_shares;
        F.count = count;
        F.base = last && base ? base->d : nullptr;
        F.base_stride = base ? base->stride() : 0;
        F.out = last ? out->d : P.p[0];
        F.out_stride = last ? out->stride() : P.stride;
        F.n = (int)cQ->h.N;
        F.lp = h->d_lp;
        LR_HIP(launch_fold(F, L1, batch, cQ->stream));
    }
    return LR_OK;
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
    if (!cP) return fail(LR_ERR_ARG, "collective: modulus P is empty (all four protocols divide by P)");
    Options parsed = cQ->opt;
    if (options) LR_TRY(options_from_public(options, &parsed));
    else parsed.apply_env();
    if (max_batch < 1 || max_batch > 65535) return fail(LR_ERR_ARG, "max_batch must be in 1 .. 65535");
    if (cQ->h.N < 8) return fail(LR_ERR_ARG, "collective: N must be at least 8 (the ternary bit planes hold N / 8 bytes, ring/ternarySampler.go:157)");
    if (cP->device != cQ->device) return fail(LR_ERR_ARG, "contexts live on different devices");
    if (cP->h.N != cQ->h.N) return fail(LR_ERR_ARG, "contexts have different ring degrees");
    LR_TRY(same_stream(cQ, cP));
    std::unique_ptr<lr_collective> h(new lr_collective());
    h->cQ = cQ;
    h->cP = cP;
    h->device = cQ->device;
    h->max_batch = max_batch;
    h->call_by_call = parsed.no_epilogue;
    h->nQ = cQ->h.L();
    h->nP = cP->h.L();
    const int rows = h->nQ + h->nP;
    if (rows > kMaxLimbs) return fail(LR_ERR_UNSUPPORTED, "collective: more than 64 limbs in Q||P");
    std::memset(&h->one, 0, sizeof h->one);
    std::memset(&h->minus_one, 0, sizeof h->minus_one);
    std::memset(&h->pmont, 0, sizeof h->pmont);
    for (int i = 0; i < rows; ++i) {     // ring/ring_context.go:119-122
        const HostContext &c = i < h->nQ ? cQ->h : cP->h;
        const int l = i < h->nQ ? i : i - h->nQ;
        h->one.v[i] = mform(1, c.q[l], c.bred[l].hi, c.bred[l].lo);
        h->minus_one.v[i] = mform(c.q[l] - 1, c.q[l], c.bred[l].hi, c.bred[l].lo);
    }
    for (int i = 0; i < h->nQ; ++i) {    // contextP.ModulusBigint mod q_i, then MForm (ring/ring.go:545-547)
        const u64 q = cQ->h.q[i];
        u64 p = 1 % q;
        for (int j = 0; j < h->nP; ++j) p = (u64)(((u128)p * (cP->h.q[j] % q)) % q);
        h->pmont.v[i] = mform(p, q, cQ->h.bred[i].hi, cQ->h.bred[i].lo);
    }
    LR_HIP(hipSetDevice(cQ->device));
    LR_TRY(lr_bext_create(cQ, cP, &h->bext));
    LR_HIP(hipMalloc((void **)&h->d_lp, (size_t)rows * sizeof(LimbParams)));
    LR_HIP(hipMemcpy(h->d_lp, cQ->d_lp, (size_t)h->nQ * sizeof(LimbParams), hipMemcpyDeviceToDevice));
    LR_HIP(hipMemcpy(h->d_lp + h->nQ, cP->d_lp, (size_t)h->nP * sizeof(LimbParams), hipMemcpyDeviceToDevice));
    const size_t N = (size_t)cQ->h.N, rand_bytes = (size_t)max_batch * (N / 4 + 2 * N);
    LR_HIP(hipMalloc((void **)&h->d_pool, (size_t)3 * max_batch * rows * N * sizeof(u64)));
    LR_HIP(hipMalloc((void **)&h->d_zero, (size_t)rows * N * sizeof(u64)));
    LR_HIP(hipMemsetAsync(h->d_zero, 0, (size_t)rows * N * sizeof(u64), cQ->stream));
    LR_HIP(hipStreamSynchronize(cQ->stream));          // the contexts may be given another stream before the first call
    LR_HIP(hipMalloc((void **)&h->d_rand, rand_bytes));
    LR_HIP(hipHostMalloc((void **)&h->h_rand, rand_bytes, 0));
    LR_HIP(hipEventCreateWithFlags(&h->staged, hipEventDisableTiming));
    *out = h.release();
    return LR_OK;
    });
}

extern "C" int lr_collective_destroy(lr_collective *h) {
    return guarded([&]() -> int {
    if (!h) return LR_OK;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();   // the handle's work may be on its context's caller-supplied stream
    delete h;
    return LR_OK;
    });
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
        return ckks_pcks_share(h, level, sk, pk0, pk1, c1, PcksRandom{u_coeff_bits, u_sign_bits, e0, e1}, batch, out0, out1, false);
    });
}
extern "C" int lr_collective_ckks_pcks_share_device(lr_collective *h, int level, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1,
                                                    const lr_poly *c1, const void *u_coeff_bits, const void *u_sign_bits, const void *e0,
                                                    const void *e1, int batch, lr_poly *out0, lr_poly *out1) {
    return guarded([&]() -> int {
        return ckks_pcks_share(h, level, sk, pk0, pk1, c1, PcksRandom{(bytes_t)u_coeff_bits, (bytes_t)u_sign_bits, (bytes_t)e0, (bytes_t)e1}, batch,
                               out0, out1, true);
    });
}
extern "C" int lr_collective_bfv_pcks_share(lr_collective *h, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1, const lr_poly *c1,
                                            const uint8_t *u_coeff_bits, const uint8_t *u_sign_bits, const uint8_t *e0, const uint8_t *e1,
                                            int batch, lr_poly *out0, lr_poly *out1) {
    return guarded([&]() -> int {
        return bfv_pcks_share(h, sk, pk0, pk1, c1, PcksRandom{u_coeff_bits, u_sign_bits, e0, e1}, batch, out0, out1, false);
    });
}
extern "C" int lr_collective_bfv_pcks_share_device(lr_collective *h, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1, const lr_poly *c1,
                                                   const void *u_coeff_bits, const void *u_sign_bits, const void *e0, const void *e1, int batch,
                                                   lr_poly *out0, lr_poly *out1) {
    return guarded([&]() -> int {
        return bfv_pcks_share(h, sk, pk0, pk1, c1, PcksRandom{(bytes_t)u_coeff_bits, (bytes_t)u_sign_bits, (bytes_t)e0, (bytes_t)e1}, batch, out0,
                              out1, true);
    });
}
extern "C" int lr_collective_aggregate(lr_collective *h, int level, const lr_poly *base, const lr_poly *const *shares, int n_shares, lr_poly *out) {
    return guarded([&]() -> int { return aggregate(h, level, base, shares, n_shares, out); });
}
