// lr_qp_handle.hpp -- what the handles that sample over Q||P from the samplers' compact bytes share: lr_bfv_encryptor, lr_ckks_encryptor,
// lr_keygen, lr_collective and lr_refresh derive from QpHandle and include this header; nothing else does.  Here, once: the two contexts and their
// limb constants side by side, the Montgomery scalars of the ternary sampler and of MulScalarBigint(P), the staging of host randomness
// through a pinned buffer, the checks every creation and every call repeat, a Context call and a transform of contextQP as two launches,
// and the one place where each of TernaryLaunch, Mul2Launch, CkksExpandLaunch and NoiseLaunch is filled.  What composes these into a
// protocol's steps stays in the handle's unit.
#pragma once
#include "lr_host.hpp"

namespace lr_host {

struct PkRandom { const unsigned char *u_coeff, *u_sign, *e0, *e1; };   // the bytes of pkEncryptor.encrypt's three samples

struct QpHandle {
    const char *name = "";                    // the prefix of the handle's refusals
    int device = 0;
    lr_context *cQ = nullptr, *cP = nullptr;  // cP == nullptr: "modulus P is empty"
    int nQ = 0, nP = 0, max_batch = 0;
    bool call_by_call = false;                // Options::no_epilogue: the reference's call-by-call shape
    LimbScalars one, minus_one;               // matrixTernaryMontgomery rows 1 and 2 (ring/ring_context.go:119-122) per limb of Q||P
    LimbScalars pmont;                        // MForm(P mod q_j) per limb of Q: MulScalarBigint's scalar (ring/ring.go:547); 0 without a cP
    LimbParams *d_lp = nullptr;               // the limb constants of contextQP: contextQ's, then contextP's
    unsigned char *d_rand = nullptr;          // the host-randomness entry points' bytes on the device ...
    unsigned char *h_rand = nullptr;          // ... and pinned
    hipEvent_t staged = nullptr;              // the last copy out of h_rand: the next call waits for it before it refills the buffer

    int rows() const { return nQ + nP; }
    int refuse(int code, const std::string &what) const { return fail(code, std::string(name) + ": " + what); }

    // the host half of a creation, after check_create and check_pair: the refusal of more than kMaxLimbs rows, the members, the scalars
    int init(const char *prefix, lr_context *ctxQ, lr_context *ctxP, int batch_limit, const Options &parsed) {
        name = prefix;
        cQ = ctxQ;
        cP = ctxP;
        device = cQ->device;
        max_batch = batch_limit;
        call_by_call = parsed.no_epilogue;
        nQ = cQ->h.L();
        nP = cP ? cP->h.L() : 0;
        if (rows() > kMaxLimbs) return refuse(LR_ERR_UNSUPPORTED, "more than 64 limbs in Q||P");
        std::memset(&one, 0, sizeof one);
        std::memset(&minus_one, 0, sizeof minus_one);
        std::memset(&pmont, 0, sizeof pmont);
        for (int i = 0; i < rows(); ++i) {     // ring/ring_context.go:119-122
            const HostContext &h = i < nQ ? cQ->h : cP->h;
            const int l = i < nQ ? i : i - nQ;
            one.v[i] = mform(1, h.q[l], h.bred[l].hi, h.bred[l].lo);
            minus_one.v[i] = mform(h.q[l] - 1, h.q[l], h.bred[l].hi, h.bred[l].lo);
        }
        for (int i = 0; cP && i < nQ; ++i) {   // contextP.ModulusBigint mod q_i, then MForm (ring/ring.go:545-547)
            const u64 q = cQ->h.q[i];
            u64 p = 1 % q;
            for (int j = 0; j < nP; ++j) p = (u64)(((u128)p * (cP->h.q[j] % q)) % q);
            pmont.v[i] = mform(p, q, cQ->h.bred[i].hi, cQ->h.bred[i].lo);
        }
        return LR_OK;
    }

    // the device half, on the handle's device: the limb constants of Q then P, and `rand_bytes` of staging with its event
    int allocate(size_t rand_bytes) {
        LR_HIP(hipMalloc((void **)&d_lp, (size_t)rows() * sizeof(LimbParams)));
        LR_HIP(hipMemcpy(d_lp, cQ->d_lp, (size_t)nQ * sizeof(LimbParams), hipMemcpyDeviceToDevice));
        if (cP) LR_HIP(hipMemcpy(d_lp + nQ, cP->d_lp, (size_t)nP * sizeof(LimbParams), hipMemcpyDeviceToDevice));
        LR_HIP(hipMalloc((void **)&d_rand, rand_bytes));
        LR_HIP(hipHostMalloc((void **)&h_rand, rand_bytes, 0));
        LR_HIP(hipEventCreateWithFlags(&staged, hipEventDisableTiming));
        return LR_OK;
    }

    // a poly of contextQ with at least `limbs` limbs and the call's batch (or, where allowed, one poly for the whole batch)
    int check_poly(const lr_poly *p, int limbs, int batch, bool broadcast, const char *what) const {
        if (p->ctx != cQ) return refuse(LR_ERR_ARG, std::string(what) + " belongs to another context");
        if (p->N != cQ->h.N || p->limbs < limbs) return refuse(LR_ERR_SHAPE, std::string(what) + " has too few limbs");
        if (p->batch != batch && !(broadcast && p->batch == 1)) return refuse(LR_ERR_SHAPE, std::string("batch differs from the batch of ") + what);
        return LR_OK;
    }

    // the caller's bytes through the pinned buffer to the device, pieces one behind the other; the caller's arrays are free on return
    int stage_random(const unsigned char *const *src, const size_t *bytes, int pieces, const unsigned char **dev) {
        LR_HIP(hipEventSynchronize(staged));               // the copy of the call before has left the pinned buffer
        size_t off = 0;
        for (int i = 0; i < pieces; ++i) {
            std::memcpy(h_rand + off, src[i], bytes[i]);
            dev[i] = d_rand + off;
            off += bytes[i];
        }
        LR_HIP(hipMemcpyAsync(d_rand, h_rand, off, hipMemcpyHostToDevice, cQ->stream));
        LR_HIP(hipEventRecord(staged, cQ->stream));
        return LR_OK;
    }
    int stage_random(const unsigned char **eb, size_t bytes) {      // one piece, its pointer replaced by the device's
        const unsigned char *src[1] = {*eb};
        return stage_random(src, &bytes, 1, eb);
    }
    int stage_random(PkRandom *R, int batch) {                       // two bit planes and two noise polys per member of the batch
        const size_t N = (size_t)cQ->h.N, plane = (size_t)batch * (N >> 3), noise = (size_t)batch * N;
        const unsigned char *src[4] = {R->u_coeff, R->u_sign, R->e0, R->e1}, *dev[4];
        const size_t bytes[4] = {plane, plane, noise, noise};
        LR_TRY(stage_random(src, bytes, 4, dev));
        *R = PkRandom{dev[0], dev[1], dev[2], dev[3]};
        return LR_OK;
    }

protected:
    ~QpHandle() {                              // (a handle is deleted as what it is: destroy_handle)
        for (void *p : {(void *)d_lp, (void *)d_rand})
            if (p) (void)hipFree(p);
        if (h_rand) (void)hipHostFree(h_rand);
        if (staged) (void)hipEventDestroy(staged);
    }
};

// what every *_create_ex refuses first, in this order: the options, max_batch, N < 8
inline int check_create(const char *prefix, const lr_context *cQ, int max_batch, const lr_options *options, Options *parsed) {
    *parsed = cQ->opt;
    if (options) LR_TRY(options_from_public(options, parsed));
    else parsed->apply_env();
    if (max_batch < 1 || max_batch > 65535) return fail(LR_ERR_ARG, "max_batch must be in 1 .. 65535");
    if (cQ->h.N < 8)
        return fail(LR_ERR_ARG, std::string(prefix) + ": N must be at least 8 (the ternary bit planes hold N / 8 bytes, ring/ternarySampler.go:157)");
    return LR_OK;
}

// ... and next: a contextP on another device or of another degree
inline int check_pair(const lr_context *cQ, const lr_context *cP) {
    if (cP && cP->device != cQ->device) return fail(LR_ERR_ARG, "contexts live on different devices");
    if (cP && cP->h.N != cQ->h.N) return fail(LR_ERR_ARG, "contexts have different ring degrees");
    return LR_OK;
}

template <class Handle>
int destroy_handle(Handle *h) {
    if (!h) return LR_OK;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();   // the handle's work may be on its context's caller-supplied stream
    delete h;
    return LR_OK;
}

// the stride of a key or a plaintext: one poly for the whole batch, or one per member
inline long long key_stride(const lr_poly *p, int batch) { return p->batch == 1 && batch > 1 ? 0 : p->stride(); }

// the words of two polys overlap: an output that is, or lies inside, an input
inline bool overlap(const lr_poly *a, const lr_poly *b) {
    const u64 *a1 = a->d + (long long)(a->batch - 1) * a->stride() + (long long)a->alloc_limbs * (long long)a->N;
    const u64 *b1 = b->d + (long long)(b->batch - 1) * b->stride() + (long long)b->alloc_limbs * (long long)b->N;
    return a->d < b1 && b->d < a1;
}

// the three pool polys of a call, back to back: [3][batch][|Q| + |P|][N]
struct Pools {
    u64 *p[3];
    long long stride, part;
};
inline Pools pools_of(const QpHandle *h, u64 *pool, int batch) {
    const long long s = (long long)h->rows() * (long long)h->cQ->h.N;
    return Pools{{pool, pool + batch * s, pool + 2 * batch * s}, s, batch * s};
}

// one Context call of contextQP (without the rows of P: of contextQ) on `batch` polys: the Q rows under contextQ, the P rows under contextP
inline int ewise_qp(QpHandle *h, bool with_p, int op, int batch, const u64 *a, long long a_stride, const u64 *b, long long b_stride, u64 *out,
                    long long out_stride) {
    const long long offP = (long long)h->nQ * (long long)h->cQ->h.N;
    LR_TRY(run_ewise(h->cQ, op, h->nQ, batch, a, a_stride, b, b_stride, out, out_stride, nullptr));
    if (!with_p) return LR_OK;
    return run_ewise(h->cP, op, h->nP, batch, a + offP, a_stride, b ? b + offP : nullptr, b_stride, out + offP, out_stride, nullptr);
}

// Context.NTT / InvNTT on `items` polys: limbs 0 .. q_limbs - 1 under contextQ and, with the rows of P, those under contextP
inline int ntt_qp(QpHandle *h, bool with_p, bool inverse, int q_limbs, int items, u64 *in, long long in_stride, u64 *out, long long out_stride) {
    LR_TRY(run_ntt(h->cQ, inverse, Rows{in, in_stride, 0, 1}, Rows{out, out_stride, 0, 1}, 0, 1, q_limbs, items));
    if (!with_p) return LR_OK;
    return run_ntt(h->cP, inverse, Rows{in, in_stride, h->nQ, 1}, Rows{out, out_stride, h->nQ, 1}, 0, 1, h->nP, items);
}

// SampleTernaryMontgomery (ring/ternarySampler.go:157-177) over rows 0 .. rows - 1 into pool poly 2
inline int ternary_qp(QpHandle *h, const Pools &P, const unsigned char *coeff_bits, const unsigned char *sign_bits, int rows, int batch) {
    TernaryLaunch T;
    T.coeff_bits = coeff_bits;
    T.sign_bits = sign_bits;
    T.out = P.p[2];
    T.out_stride = P.stride;
    T.n = (int)h->cQ->h.N;
    T.one = h->one;
    T.minus_one = h->minus_one;
    LR_HIP(launch_bfv_ternary(T, rows, batch, h->cQ->stream));
    return LR_OK;
}

// both products of pkEncryptor.encrypt in one pass over u: pool poly 2 times pk0 and pk1 into pool polys 0 and 1, rows 0 .. rows - 1 in one launch
inline int mul2_qp(QpHandle *h, const Pools &P, const lr_poly *pk0, const lr_poly *pk1, int rows, int batch) {
    Mul2Launch M;
    M.a = P.p[2]; M.a_stride = P.stride;
    M.b0 = pk0->d; M.b0_stride = key_stride(pk0, batch);
    M.b1 = pk1->d; M.b1_stride = key_stride(pk1, batch);
    M.out0 = P.p[0]; M.out1 = P.p[1];
    M.out0_stride = M.out1_stride = P.stride;
    M.n = (int)h->cQ->h.N;
    M.lp = h->d_lp;
    LR_HIP(launch_mul2(M, rows, batch, h->cQ->stream));
    return LR_OK;
}

inline LimbScalars from_row(const LimbScalars &v, int row0) {
    LimbScalars r;
    std::memset(&r, 0, sizeof r);
    for (int i = row0; i < kMaxLimbs; ++i) r.v[i - row0] = v.v[i];
    return r;
}

// SampleTernaryMontgomery and / or KYSampler.Sample as a forward transform's operands (the q of (0, sign 0) written as 0) on rows
// row0 .. row0 + rows - 1 of Q||P: `ternary` + `noises` parts of `items` polys from `out` (a poly's row 0) on, `part` apart
inline int expand_qp(QpHandle *h, int row0, int rows, int ternary, const unsigned char *u_coeff, const unsigned char *u_sign, int noises,
                     const unsigned char *e0, const unsigned char *e1, u64 *out, long long stride, long long part, int items) {
    CkksExpandLaunch X;
    std::memset(&X, 0, sizeof X);
    X.coeff_bits = u_coeff;
    X.sign_bits = u_sign;
    X.e[0] = e0;
    X.e[1] = e1;
    X.out = out + (long long)row0 * (long long)h->cQ->h.N;
    X.out_stride = stride;
    X.part_stride = part;
    X.n = (int)h->cQ->h.N;
    X.ternary = ternary;
    X.noises = noises;
    X.one = from_row(h->one, row0);
    X.minus_one = from_row(h->minus_one, row0);
    X.lp = h->d_lp + row0;
    LR_HIP(launch_ckks_expand(X, rows, items, h->cQ->stream));
    return LR_OK;
}

// KYSampler.Sample (ring/gaussianSampler.go:230-251) into `comps` polys x[k] over rows 0 .. rows - 1 (add = 0: the residue q_j of
// (0, sign 0) as the reference stores it), or SampleAndAdd / Sample + Context.Add on them (add = 1).  With add = 1 the sums go to dst[k]
// where dst is given, and `plus` (the Context.Add of the plaintext that ends encrypt) rides on component 0.
inline int noise_qp(QpHandle *h, int add, int comps, const unsigned char *const *eb, u64 *const *x, long long stride, int rows, int batch,
                    lr_poly *const *dst = nullptr, const lr_poly *plus = nullptr) {
    NoiseLaunch L;
    std::memset(&L, 0, sizeof L);
    for (int k = 0; k < comps; ++k) {
        L.x[k] = add ? x[k] : nullptr;
        L.x_stride[k] = stride;
        L.out[k] = dst ? dst[k]->d : x[k];
        L.out_stride[k] = dst ? dst[k]->stride() : stride;
        L.e[k] = eb[k];
    }
    if (plus) {
        L.plus[0] = plus->d;
        L.plus_stride[0] = key_stride(plus, batch);
    }
    L.n = (int)h->cQ->h.N;
    L.add = add;
    L.lp = h->d_lp;
    LR_HIP(launch_bfv_noise(L, comps, rows, batch, h->cQ->stream));
    return LR_OK;
}

// the same words, poly for poly: what an element-wise pass may read and write at once
inline bool same_poly(const lr_poly *a, const lr_poly *b) { return a->d == b->d && a->batch == b->batch && (a->batch == 1 || a->stride() == b->stride()); }

// the outputs of a share call against its inputs and against each other; output 0 may be the input `may_be` as a whole poly
inline int check_outputs(const QpHandle *h, const lr_poly *const *outs, int n_outs, const lr_poly *const *ins, int n_ins, const lr_poly *may_be = nullptr) {
    for (int o = 0; o < n_outs; ++o) {
        for (int i = 0; i < n_ins; ++i)
            if (overlap(outs[o], ins[i]) && !(ins[i] == may_be && o == 0 && same_poly(outs[o], ins[i])))
                return h->refuse(LR_ERR_ARG, "an output shares memory with an input");
        for (int j = 0; j < o; ++j)
            if (overlap(outs[o], outs[j])) return h->refuse(LR_ERR_ARG, "the two outputs share memory");
    }
    return LR_OK;
}

// what every call of lr_collective and lr_refresh refuses first: the level, the batch, two contexts on two streams
inline int check_call(const QpHandle *h, int level, int batch) {
    if (level < 0 || level + 1 > h->nQ) return h->refuse(LR_ERR_SHAPE, "level out of range");
    if (batch < 1) return h->refuse(LR_ERR_SHAPE, "batch must be at least 1");
    if (batch > h->max_batch) return h->refuse(LR_ERR_SHAPE, "batch exceeds the handle's max_batch");
    return h->cP ? same_stream(h->cQ, h->cP) : LR_OK;
}

// The n-ary fold behind every Aggregate*: acc = shares[0]; acc = CRed(acc + shares[k]) in the shares' order; out = base ? CRed(base + acc) :
// acc, over limbs 0 .. q_limbs - 1 of Q and, with_p, the rows of P.  `pool` holds one poly over Q||P per member of the batch.  The checks
// that do not depend on which rows are folded are here; the level (lr_collective, lr_refresh) or the batch (lr_setup) is the caller's.
inline int fold_rows(QpHandle *h, u64 *pool, int q_limbs, bool with_p, const lr_poly *base, const lr_poly *const *shares, int n_shares, lr_poly *out) {
    const int batch = out->batch, limbs = q_limbs + (with_p ? h->nP : 0);
    LR_TRY(h->check_poly(out, limbs, batch, false, "the output"));
    if (base) {
        LR_TRY(h->check_poly(base, limbs, batch, false, "the base"));
        if (overlap(out, base) && !same_poly(out, base)) return h->refuse(LR_ERR_ARG, "the output overlaps the base without being it");
    }
    for (int k = 0; k < n_shares; ++k) {
        if (!shares[k]) return fail(LR_ERR_ARG, "null argument");
        LR_TRY(h->check_poly(shares[k], limbs, batch, false, "a share"));
        if (overlap(out, shares[k]) && !same_poly(out, shares[k])) return h->refuse(LR_ERR_ARG, "the output overlaps a share without being it");
    }
    LR_HIP(hipSetDevice(h->device));
    lr_context *cQ = h->cQ;
    const Pools P = pools_of(h, pool, batch);
    const auto add = [&](int op, const u64 *a, long long a_stride, const u64 *b, long long b_stride, u64 *dst, long long dst_stride) -> int {
        if (with_p) return ewise_qp(h, true, op, batch, a, a_stride, b, b_stride, dst, dst_stride);
        return run_ewise(cQ, op, q_limbs, batch, a, a_stride, b, b_stride, dst, dst_stride, nullptr);
    };
    if (h->call_by_call) {     // n_shares - 1 Context.Add calls, then KeySwitch's; the running sum lives in the pool: out may be base or a share
        const u64 *acc = shares[0]->d;
        long long acc_stride = shares[0]->stride();
        for (int k = 1; k < n_shares; ++k) {
            const bool last = k == n_shares - 1 && !base;
            u64 *dst = last ? out->d : P.p[0];
            const long long dst_stride = last ? out->stride() : P.stride;
            LR_TRY(add(LR_ADD, acc, acc_stride, shares[k]->d, shares[k]->stride(), dst, dst_stride));
            acc = dst;
            acc_stride = dst_stride;
        }
        if (base) return add(LR_ADD, base->d, base->stride(), acc, acc_stride, out->d, out->stride());
        if (n_shares == 1) return add(LR_COPY, acc, acc_stride, nullptr, 0, out->d, out->stride());
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
        LR_HIP(launch_fold(F, limbs, batch, cQ->stream));
    }
    return LR_OK;
}

// AggregateShares over n_shares parties and, with a base, KeySwitch's Add (dckks/keyswitching.go:99-108 and its three twins; Aggregate of
// both RefreshProtocols): lr_collective_aggregate and lr_refresh_aggregate, over limbs 0 .. level of Q
inline int fold_shares(QpHandle *h, u64 *pool, int level, const lr_poly *base, const lr_poly *const *shares, int n_shares, lr_poly *out) {
    if (!h || !shares || !out) return fail(LR_ERR_ARG, "null argument");
    if (n_shares < 1) return h->refuse(LR_ERR_SHAPE, "n_shares must be at least 1");
    LR_TRY(check_call(h, level, out->batch));
    return fold_rows(h, pool, level + 1, false, base, shares, n_shares, out);
}

}  // namespace lr_host
