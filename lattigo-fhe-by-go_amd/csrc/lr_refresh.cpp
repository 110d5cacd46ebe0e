// lr_refresh.cpp -- C ABI: lr_refresh, the collective Refresh of dckks and dbfv for a batch of ciphertexts on the device:
// dckks/public_refresh.go GenShares (:43-95, after the drawing of the mask and the noise), Aggregate (:98), Decrypt (:103), Recode
// (:108-139), Recrypt (:142-147); dbfv/public_refresh.go GenShares (:105-160), Aggregate (:163), Decrypt (:169), Recode (:174-179), Recrypt
// (:182-190), Finalize (:193-197), lift (:199-205).  The noise arrives in the encryptors' compact form, the CKKS mask as word planes of
// signed multi-word integers, the BFV mask as one row of values below t.  Kernels: lr_refresh.hip, the expansions of lr_ckks_encrypt.hip
// and lr_bfv_encrypt.hip, launch_fold, launch_bfv_lift and launch_simple_scale; the ModDowns are lr_bext's.
// The launchers of lr_refresh.hip have their stand-in for the host sanitizer build in tests/cpp/hipstub/stub_refresh.cpp; what the unit
// shares with lr_keygen.cpp and lr_collective.cpp is lr_qp_handle.hpp.
#include "lr_qp_handle.hpp"

// what the two NewRefreshProtocol constructors build (dckks/public_refresh.go:23-35, dbfv/public_refresh.go:79-96); the contexts, the
// scalars and the staging of the host-randomness entry points are QpHandle's
struct lr_refresh : lr_host::QpHandle {
    u64 t = 0;                                // the plaintext modulus; 0: CKKS entry points only
    lr_bext *bext = nullptr;                  // NewFastBasisExtender(contextQ, contextP), owned; with a cP only
    lr_simple_scaler *scaler = nullptr;       // NewSimpleScaler(t, contextQ) of dbfv Recode (:175), owned; with t only
    u64 *d_pool = nullptr;                    // three polys over Q||P for max_batch ciphertexts
    u64 *d_row = nullptr;                     // [max_batch][N]: SimpleScaler's output in front of lift
    u64 *d_delta = nullptr;                   // deltaMont (dbfv/dbfv.go), [|Q|]
    u64 *d_tab = nullptr;                     // Recode's constants: qmod [|Q|][|Q|], ginv [|Q|], then per levelStart hdig [|Q|] and qls [|Q|]
    LimbScalars two64;                        // 2^64 mod q_i
    std::vector<int> words;                   // per levelStart: ceil(bitlen(Q_levelStart) / 64)
    ~lr_refresh() {
        for (void *p : {(void *)d_pool, (void *)d_row, (void *)d_delta, (void *)d_tab})
            if (p) (void)hipFree(p);
        if (scaler) lr_simple_scaler_destroy(scaler);
        if (bext) lr_bext_destroy(bext);
    }
};

namespace lr_host {
namespace {

// a non-negative integer on little-endian 64-bit words: the products Q_levelStart of the constructor, nothing per call
typedef std::vector<u64> Big;
void big_mul(Big &a, u64 m) {
    u64 carry = 0;
    for (u64 &w : a) {
        const u128 p = (u128)w * m + carry;
        w = (u64)p;
        carry = (u64)(p >> 64);
    }
    if (carry) a.push_back(carry);
}
u64 big_divmod(Big &a, u64 m) {               // a /= m, returns the remainder
    u64 rem = 0;
    for (size_t i = a.size(); i-- > 0;) {
        const u128 cur = ((u128)rem << 64) | a[i];
        a[i] = (u64)(cur / m);
        rem = (u64)(cur % m);
    }
    while (a.size() > 1 && a.back() == 0) a.pop_back();
    return rem;
}
void big_shr1(Big &a) {
    for (size_t i = 0; i < a.size(); ++i) a[i] = (a[i] >> 1) | (i + 1 < a.size() ? a[i + 1] << 63 : 0);
    while (a.size() > 1 && a.back() == 0) a.pop_back();
}
int big_bitlen(const Big &a) { return a.back() ? 64 * (int)a.size() - __builtin_clzll(a.back()) : 0; }

u64 mulmod(u64 a, u64 b, u64 q) { return (u64)(((u128)a * b) % q); }
u64 invmod(u64 a, u64 q) {                    // q prime
    u64 r = 1 % q, e = q - 2;
    for (a %= q; e; e >>= 1, a = mulmod(a, a, q))
        if (e & 1) r = mulmod(r, a, q);
    return r;
}

int check_words(const lr_refresh *h, int level_start) {
    if (h->words[level_start] > kCkksCrtMaxWords) return h->refuse(LR_ERR_UNSUPPORTED, "Q_levelStart exceeds 2048 bits, the limit of the multi-word masks");
    return LR_OK;
}

int check_bfv(const lr_refresh *h) {
    if (!h->cP || !h->t) return h->refuse(LR_ERR_ARG, "the handle was created without P or without t (CKKS entry points only)");
    return LR_OK;
}

Rows rows_at(const u64 *base, long long stride, int limb0) { return Rows{const_cast<u64 *>(base), stride, limb0, 1}; }

// SetCoefficientsBigintLvl(limbs - 1, mask, out) (:66, :68)
int reduce_mask(lr_refresh *h, const u64 *mask, int words, int limbs, u64 *out, long long out_stride, int batch) {
    RefreshMaskLaunch M;
    M.mask = mask;
    M.out = out;
    M.out_stride = out_stride;
    M.n = (int)h->cQ->h.N;
    M.words = words;
    M.two64 = h->two64;
    M.lp = h->d_lp;
    LR_HIP(launch_refresh_mask(M, limbs, batch, h->cQ->stream));
    return LR_OK;
}

// RefreshProtocol.GenShares of dckks (dckks/public_refresh.go:66-92)
int ckks_shares(lr_refresh *h, int ls, const lr_poly *sk, const lr_poly *c1, const lr_poly *crs, const u64 *mask, const unsigned char *e0,
                const unsigned char *e1, int batch, lr_poly *dec, lr_poly *rec, bool on_device) {
    if (!h || !sk || !c1 || !crs || !mask || !e0 || !e1 || !dec || !rec) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_call(h, ls, batch));
    LR_TRY(check_words(h, ls));
    const int nQ = h->nQ, L1 = ls + 1, W = h->words[ls];
    LR_TRY(h->check_poly(sk, nQ, batch, true, "the secret key"));
    LR_TRY(h->check_poly(c1, L1, batch, false, "the ciphertext"));
    LR_TRY(h->check_poly(crs, nQ, batch, false, "the common reference poly"));
    LR_TRY(h->check_poly(dec, L1, batch, false, "the decryption share"));
    LR_TRY(h->check_poly(rec, nQ, batch, false, "the recryption share"));
    const lr_poly *outs[2] = {dec, rec}, *ins[3] = {sk, c1, crs};
    LR_TRY(check_outputs(h, outs, 2, ins, 3));
    if (on_device && ((uintptr_t)mask & 7)) return h->refuse(LR_ERR_ARG, "the mask is not aligned to 8 bytes");
    LR_HIP(hipSetDevice(h->device));
    lr_context *cQ = h->cQ;
    const size_t N = (size_t)cQ->h.N;
    if (!on_device) {
        const unsigned char *src[3] = {(const unsigned char *)mask, e0, e1}, *dev[3];
        const size_t bytes[3] = {(size_t)batch * (size_t)W * N * sizeof(u64), (size_t)batch * N, (size_t)batch * N};
        LR_TRY(h->stage_random(src, bytes, 3, dev));
        mask = (const u64 *)dev[0];
        e0 = dev[1];
        e1 = dev[2];
    }
    const Pools P = pools_of(h, h->d_pool, batch);
    const long long sks = key_stride(sk, batch);
    if (h->call_by_call) {
        LR_TRY(reduce_mask(h, mask, W, L1, dec->d, dec->stride(), batch));                                            // :66
        LR_TRY(reduce_mask(h, mask, W, nQ, rec->d, rec->stride(), batch));                                            // :68
        LR_TRY(run_ntt(cQ, false, rows_at(dec->d, dec->stride(), 0), rows_at(dec->d, dec->stride(), 0), 0, 1, L1, batch));   // :74
        LR_TRY(run_ntt(cQ, false, rows_at(rec->d, rec->stride(), 0), rows_at(rec->d, rec->stride(), 0), 0, 1, nQ, batch));   // :75
        LR_TRY(run_ewise(cQ, LR_MUL_MONT_AND_ADD, L1, batch, sk->d, sks, c1->d, c1->stride(), dec->d, dec->stride(), nullptr));   // :78
        LR_TRY(run_ewise(cQ, LR_MUL_MONT_AND_ADD, nQ, batch, sk->d, sks, crs->d, crs->stride(), rec->d, rec->stride(), nullptr)); // :81
        const unsigned char *eb[2] = {e0, e1};
        lr_poly *share[2] = {dec, rec};
        const int limbs[2] = {L1, nQ};
        for (int k = 0; k < 2; ++k) {                                                                                 // :84-85, :88-89
            LR_TRY(expand_qp(h, 0, nQ, 0, nullptr, nullptr, 1, eb[k], nullptr, P.p[0], P.stride, P.part, batch));     // SampleNTT over all of Q
            LR_TRY(run_ntt(cQ, false, rows_at(P.p[0], P.stride, 0), rows_at(P.p[0], P.stride, 0), 0, 1, nQ, batch));
            LR_TRY(run_ewise(cQ, LR_ADD, limbs[k], batch, share[k]->d, share[k]->stride(), P.p[0], P.stride, share[k]->d, share[k]->stride(), nullptr));
        }
        return run_ewise(cQ, LR_NEG, nQ, batch, rec->d, rec->stride(), nullptr, 0, rec->d, rec->stride(), nullptr);   // :92
    }
    // pool 0 = e0 on limbs 0 .. ls, pool 1 = the mask over all of Q, reduced once, pool 2 = e1 over all of Q; one transform over the three
    // on limbs 0 .. ls and one over the last two above; then one pass per row for both shares
    LR_TRY(reduce_mask(h, mask, W, nQ, P.p[1], P.stride, batch));
    LR_TRY(expand_qp(h, 0, L1, 0, nullptr, nullptr, 2, e0, e1, P.p[0], P.stride, 2 * P.part, batch));
    if (L1 < nQ) LR_TRY(expand_qp(h, L1, nQ - L1, 0, nullptr, nullptr, 1, e1, nullptr, P.p[2], P.stride, 0, batch));
    LR_TRY(run_ntt(cQ, false, rows_at(P.p[0], P.stride, 0), rows_at(P.p[0], P.stride, 0), 0, 1, L1, 3 * batch));
    if (L1 < nQ) LR_TRY(run_ntt(cQ, false, rows_at(P.p[1], P.stride, L1), rows_at(P.p[1], P.stride, L1), L1, 1, nQ - L1, 2 * batch));
    RefreshCkksShareLaunch S;
    S.e0 = P.p[0]; S.mask = P.p[1]; S.e1 = P.p[2];
    S.r_stride = P.stride;
    S.sk = sk->d; S.sk_stride = sks;
    S.c1 = c1->d; S.c1_stride = c1->stride();
    S.crs = crs->d; S.crs_stride = crs->stride();
    S.dec = dec->d; S.dec_stride = dec->stride();
    S.rec = rec->d; S.rec_stride = rec->stride();
    S.n = (int)N;
    S.dec_limbs = L1;
    S.lp = h->d_lp;
    LR_HIP(launch_refresh_ckks_share(S, nQ, batch, cQ->stream));
    return LR_OK;
}

int recode_launch(lr_refresh *h, int ls, int row0, const u64 *in, long long in_stride, u64 *out, long long out_stride, int batch) {
    const int nQ = h->nQ;
    RefreshRecodeLaunch R;
    R.in = in; R.in_stride = in_stride;
    R.out = out; R.out_stride = out_stride;
    R.n = (int)h->cQ->h.N;
    R.ls = ls;
    R.row0 = row0;
    R.limbs = nQ;
    R.qmod = h->d_tab;
    R.ginv = h->d_tab + (size_t)nQ * nQ;
    R.hdig = h->d_tab + (size_t)nQ * nQ + nQ + (size_t)ls * 2 * nQ;
    R.qls = R.hdig + nQ;
    R.lp = h->d_lp;
    LR_HIP(launch_refresh_recode(R, batch, h->cQ->stream));
    return LR_OK;
}

// Recode (:108-139) of `in` (NTT domain, limbs 0 .. ls) into `out` over all of Q; `in` may be `out`.  Pool 0 is the scratch.
int recode_core(lr_refresh *h, int ls, const u64 *in, long long in_stride, u64 *out, long long out_stride, int batch) {
    lr_context *cQ = h->cQ;
    const Pools P = pools_of(h, h->d_pool, batch);
    const int nQ = h->nQ, L1 = ls + 1;
    if (!h->call_by_call && L1 == nQ)       // levelStart = L: no row is added, the result is the input
        return in != out ? run_ewise(cQ, LR_COPY, L1, batch, in, in_stride, nullptr, 0, out, out_stride, nullptr) : LR_OK;
    LR_TRY(run_ntt(cQ, true, rows_at(in, in_stride, 0), rows_at(P.p[0], P.stride, 0), 0, 1, L1, batch));             // :112
    if (h->call_by_call) {
        LR_TRY(recode_launch(h, ls, 0, P.p[0], P.stride, out, out_stride, batch));                                    // :114-136, every row
        return run_ntt(cQ, false, rows_at(out, out_stride, 0), rows_at(out, out_stride, 0), 0, 1, nQ, batch);         // :138
    }
    // rows 0 .. ls of the result are v mod q_i = the input's own residues, transformed back to what they were: they are copied, and only
    // the new rows are computed and transformed
    LR_TRY(recode_launch(h, ls, L1, P.p[0], P.stride, out, out_stride, batch));
    LR_TRY(run_ntt(cQ, false, rows_at(out, out_stride, L1), rows_at(out, out_stride, L1), L1, 1, nQ - L1, batch));
    if (in != out) LR_TRY(run_ewise(cQ, LR_COPY, L1, batch, in, in_stride, nullptr, 0, out, out_stride, nullptr));
    return LR_OK;
}

int ckks_recode(lr_refresh *h, int ls, const lr_poly *in, lr_poly *out) {
    if (!h || !in || !out) return fail(LR_ERR_ARG, "null argument");
    const int batch = out->batch;
    LR_TRY(check_call(h, ls, batch));
    LR_TRY(check_words(h, ls));
    LR_TRY(h->check_poly(in, ls + 1, batch, false, "the input"));
    LR_TRY(h->check_poly(out, h->nQ, batch, false, "the output"));
    if (overlap(out, in) && !same_poly(out, in)) return h->refuse(LR_ERR_ARG, "the output overlaps the input without being it");
    LR_HIP(hipSetDevice(h->device));
    return recode_core(h, ls, in->d, in->stride(), out->d, out->stride(), batch);
}

// Decrypt (:103-105), Recode (:108-139) and Recrypt's Add (:144)
int ckks_finalize(lr_refresh *h, int ls, const lr_poly *c0, const lr_poly *dec, const lr_poly *rec, lr_poly *out0) {
    if (!h || !c0 || !dec || !rec || !out0) return fail(LR_ERR_ARG, "null argument");
    const int batch = out0->batch;
    LR_TRY(check_call(h, ls, batch));
    LR_TRY(check_words(h, ls));
    const int nQ = h->nQ, L1 = ls + 1;
    LR_TRY(h->check_poly(c0, L1, batch, false, "the ciphertext"));
    LR_TRY(h->check_poly(dec, L1, batch, false, "the decryption share"));
    LR_TRY(h->check_poly(rec, nQ, batch, false, "the recryption share"));
    LR_TRY(h->check_poly(out0, nQ, batch, false, "the output"));
    const lr_poly *outs[1] = {out0}, *ins[3] = {c0, dec, rec};
    LR_TRY(check_outputs(h, outs, 1, ins, 3, c0));
    LR_HIP(hipSetDevice(h->device));
    lr_context *cQ = h->cQ;
    const Pools P = pools_of(h, h->d_pool, batch);
    LR_TRY(run_ewise(cQ, LR_ADD, L1, batch, c0->d, c0->stride(), dec->d, dec->stride(), P.p[1], P.stride, nullptr));  // :104
    LR_TRY(recode_core(h, ls, P.p[1], P.stride, P.p[1], P.stride, batch));
    return run_ewise(cQ, LR_ADD, nQ, batch, P.p[1], P.stride, rec->d, rec->stride(), out0->d, out0->stride(), nullptr);   // :144
}

int lift_launch(lr_refresh *h, const u64 *row, lr_poly *dec, lr_poly *rec, const lr_poly *plus, int batch) {
    RefreshBfvLiftLaunch F;
    F.row = row;
    F.plus = plus ? plus->d : nullptr; F.plus_stride = plus ? plus->stride() : 0;
    F.dec = dec->d; F.dec_stride = dec->stride();
    F.rec = rec ? rec->d : nullptr; F.rec_stride = rec ? rec->stride() : 0;
    F.n = (int)h->cQ->h.N;
    F.delta_mont = h->d_delta;
    F.lp = h->d_lp;
    LR_HIP(launch_refresh_bfv_lift(F, h->nQ, batch, h->cQ->stream));
    return LR_OK;
}

// RefreshProtocol.GenShares of dbfv (dbfv/public_refresh.go:105-160), as the first call on a fresh protocol object: hP starts at zero
int bfv_shares(lr_refresh *h, const lr_poly *sk, const lr_poly *c1, const lr_poly *crs, const u64 *mask, const unsigned char *e0,
               const unsigned char *e1, int batch, lr_poly *dec, lr_poly *rec, bool on_device) {
    if (!h || !sk || !c1 || !crs || !mask || !e0 || !e1 || !dec || !rec) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_bfv(h));
    const int nQ = h->nQ, rows = h->rows(), level = nQ - 1;
    LR_TRY(check_call(h, level, batch));
    LR_TRY(h->check_poly(sk, rows, batch, true, "the secret key"));
    LR_TRY(h->check_poly(c1, nQ, batch, false, "the ciphertext"));
    LR_TRY(h->check_poly(crs, rows, batch, false, "the common reference poly"));
    LR_TRY(h->check_poly(dec, nQ, batch, false, "the decryption share"));
    LR_TRY(h->check_poly(rec, nQ, batch, false, "the recryption share"));
    const lr_poly *outs[2] = {dec, rec}, *ins[3] = {sk, c1, crs};
    LR_TRY(check_outputs(h, outs, 2, ins, 3));
    if (on_device && ((uintptr_t)mask & 15)) return h->refuse(LR_ERR_ARG, "the mask is not aligned to 16 bytes");
    LR_HIP(hipSetDevice(h->device));
    lr_context *cQ = h->cQ;
    const size_t N = (size_t)cQ->h.N;
    if (!on_device) {
        const unsigned char *src[3] = {(const unsigned char *)mask, e0, e1}, *dev[3];
        const size_t bytes[3] = {(size_t)batch * N * sizeof(u64), (size_t)batch * N, (size_t)batch * N};
        LR_TRY(h->stage_random(src, bytes, 3, dev));
        mask = (const u64 *)dev[0];
        e0 = dev[1];
        e1 = dev[2];
    }
    const Pools P = pools_of(h, h->d_pool, batch);
    const long long sks = key_stride(sk, batch);
    const Rows hP0{P.p[0], P.stride, nQ, 1}, hP1{P.p[1], P.stride, nQ, 1};
    if (h->call_by_call) {
        const Rows q2{P.p[2], P.stride, 0, 1};
        LR_TRY(run_ntt(cQ, false, rows_at(c1->d, c1->stride(), 0), rows_at(P.p[0], P.stride, 0), 0, 1, nQ, batch));   // :116
        LR_TRY(run_ewise(cQ, LR_MUL_MONT, nQ, batch, sk->d, sks, P.p[0], P.stride, P.p[2], P.stride, nullptr));       // :117
        LR_TRY(run_ntt(cQ, true, q2, q2, 0, 1, nQ, batch));                                                           // :119
        LR_TRY(run_ewise(cQ, LR_MUL_SCALAR_LIMBS, nQ, batch, P.p[2], P.stride, nullptr, 0, P.p[2], P.stride, &h->pmont));   // :122
        LR_TRY(noise_qp(h, 0, 1, &e0, &P.p[0], P.stride, rows, batch));                                               // :125 Sample over Q||P
        LR_TRY(run_ewise(cQ, LR_ADD, nQ, batch, P.p[2], P.stride, P.p[0], P.stride, P.p[2], P.stride, nullptr));      // :126
        // :128-134: hP = the rows of P as they are, p_j of (0, sign 0) included
        LR_TRY(moddown_pq_core(h->bext, level, P.p[2], P.stride, hP0, batch, dec, false));                            // :137
        LR_TRY(ntt_qp(h, true, false, nQ, batch, crs->d, crs->stride(), P.p[0], P.stride));                           // :140
        LR_TRY(ewise_qp(h, true, LR_MUL_MONT, batch, sk->d, sks, P.p[0], P.stride, P.p[1], P.stride));                // :141
        LR_TRY(ewise_qp(h, true, LR_NEG, batch, P.p[1], P.stride, nullptr, 0, P.p[1], P.stride));                     // :142
        LR_TRY(ntt_qp(h, true, true, nQ, batch, P.p[1], P.stride, P.p[1], P.stride));                                 // :143
        LR_TRY(noise_qp(h, 0, 1, &e1, &P.p[0], P.stride, rows, batch));                                               // :146 SampleAndAdd
        LR_TRY(ewise_qp(h, true, LR_ADD, batch, P.p[1], P.stride, P.p[0], P.stride, P.p[1], P.stride));
        LR_TRY(moddown_pq_core(h->bext, level, P.p[1], P.stride, hP1, batch, rec, false));                            // :149
        LR_HIP(launch_bfv_lift(mask, (int)N, P.p[0], P.stride, nQ, h->d_lp, h->d_delta, batch, cQ->stream));          // :153
        LR_TRY(run_ewise(cQ, LR_ADD, nQ, batch, dec->d, dec->stride(), P.p[0], P.stride, dec->d, dec->stride(), nullptr));   // :156
        return run_ewise(cQ, LR_SUB, nQ, batch, rec->d, rec->stride(), P.p[0], P.stride, rec->d, rec->stride(), nullptr);    // :159
    }
    // pool 0 = NTT(c1) on Q, pool 1 = NTT(crs) on Q||P; both products in one pass, one inverse transform over the two on the rows of Q
    LR_TRY(run_ntt(cQ, false, rows_at(c1->d, c1->stride(), 0), rows_at(P.p[0], P.stride, 0), 0, 1, nQ, batch));
    LR_TRY(ntt_qp(h, true, false, nQ, batch, crs->d, crs->stride(), P.p[1], P.stride));
    RefreshBfvProductLaunch M;
    M.sk = sk->d; M.sk_stride = sks;
    M.a = P.p[0]; M.b = P.p[1];
    M.stride = P.stride;
    M.n = (int)N;
    M.nQ = nQ;
    M.pmont = h->pmont;
    M.lp = h->d_lp;
    LR_HIP(launch_refresh_bfv_product(M, rows, batch, cQ->stream));
    LR_TRY(run_ntt(cQ, true, rows_at(P.p[0], P.stride, 0), rows_at(P.p[0], P.stride, 0), 0, 1, nQ, 2 * batch));       // (the two pools are back to back)
    LR_TRY(run_ntt(h->cP, true, hP1, hP1, 0, 1, h->nP, batch));
    LR_TRY(noise_qp(h, 1, 1, &e0, &P.p[0], P.stride, nQ, batch));                           // CRed(x + residue) on the rows of Q
    // the residue on the rows of P, p_j written as 0: no bit of the ModDown's output changes (tests/test_oracle_refresh.py)
    LR_TRY(expand_qp(h, nQ, h->nP, 0, nullptr, nullptr, 1, e0, nullptr, P.p[0], P.stride, 0, batch));
    LR_TRY(noise_qp(h, 1, 1, &e1, &P.p[1], P.stride, rows, batch));
    LR_TRY(moddown_pq_core(h->bext, level, P.p[0], P.stride, hP0, batch, dec, false));
    LR_TRY(moddown_pq_core(h->bext, level, P.p[1], P.stride, hP1, batch, rec, false));
    return lift_launch(h, mask, dec, rec, nullptr, batch);
}

// Finalize (:193-197): Decrypt (:170), Recode (:175-178), Recrypt (:185-188)
int bfv_finalize(lr_refresh *h, const lr_poly *c0, const lr_poly *crs, const lr_poly *dec, const lr_poly *rec, lr_poly *out0, lr_poly *out1) {
    if (!h || !c0 || !crs || !dec || !rec || !out0 || !out1) return fail(LR_ERR_ARG, "null argument");
    LR_TRY(check_bfv(h));
    const int nQ = h->nQ, level = nQ - 1, batch = out0->batch;
    LR_TRY(check_call(h, level, batch));
    LR_TRY(h->check_poly(c0, nQ, batch, false, "the ciphertext"));
    LR_TRY(h->check_poly(crs, h->rows(), batch, false, "the common reference poly"));
    LR_TRY(h->check_poly(dec, nQ, batch, false, "the decryption share"));
    LR_TRY(h->check_poly(rec, nQ, batch, false, "the recryption share"));
    LR_TRY(h->check_poly(out0, nQ, batch, false, "the output"));
    LR_TRY(h->check_poly(out1, nQ, batch, false, "the output"));
    const lr_poly *outs[2] = {out0, out1}, *ins[4] = {c0, crs, dec, rec};
    LR_TRY(check_outputs(h, outs, 2, ins, 4, c0));
    LR_HIP(hipSetDevice(h->device));
    lr_context *cQ = h->cQ;
    const long long N = (long long)cQ->h.N;
    const Pools P = pools_of(h, h->d_pool, batch);
    const lr_simple_scaler *s = h->scaler;
    ScaleLaunch S;
    S.in = P.p[0]; S.in_stride = P.stride;
    S.wi = s->d_wi; S.ti = s->d_ti;
    S.t = s->h.t; S.add_param = s->h.add_param; S.mul_param = s->h.mul_param;
    S.pow2 = s->h.pow2 ? 1 : 0;
    S.limbs_in = nQ;
    S.n = (int)N;
    LR_TRY(run_ewise(cQ, LR_ADD, nQ, batch, c0->d, c0->stride(), dec->d, dec->stride(), P.p[0], P.stride, nullptr));  // :170
    if (h->call_by_call) {
        S.out = P.p[0]; S.out_stride = P.stride; S.limbs_out = nQ;
        LR_HIP(launch_simple_scale(S, batch, cQ->stream));                                                            // :177, every row
        LR_TRY(run_ewise(cQ, LR_COPY, 1, batch, P.p[0], P.stride, nullptr, 0, h->d_row, N, nullptr));                 // lift reads Coeffs[0]
        LR_HIP(launch_bfv_lift(h->d_row, (int)N, P.p[1], P.stride, nQ, h->d_lp, h->d_delta, batch, cQ->stream));      // :178
        LR_TRY(run_ewise(cQ, LR_ADD, nQ, batch, P.p[1], P.stride, rec->d, rec->stride(), out0->d, out0->stride(), nullptr));   // :185
    } else {
        S.out = h->d_row; S.out_stride = N; S.limbs_out = 1;
        LR_HIP(launch_simple_scale(S, batch, cQ->stream));
        LR_TRY(lift_launch(h, h->d_row, out0, nullptr, rec, batch));
    }
    return moddown_pq_core(h->bext, level, crs->d, crs->stride(), rows_at(crs->d, crs->stride(), nQ), batch, out1, false);   // :188
}

}  // namespace
}  // namespace lr_host

extern "C" int lr_refresh_create(lr_context *cQ, lr_context *cP, uint64_t t, int max_batch, lr_refresh **out) {
    return lr_refresh_create_ex(cQ, cP, t, max_batch, nullptr, out);
}

extern "C" int lr_refresh_create_ex(lr_context *cQ, lr_context *cP, uint64_t t, int max_batch, const lr_options *options, lr_refresh **out) {
    return guarded([&]() -> int {
    if (!cQ || !out) return fail(LR_ERR_ARG, "null argument");
    *out = nullptr;
    const char *name = "refresh";
    Options parsed;
    LR_TRY(check_create(name, cQ, max_batch, options, &parsed));
    LR_TRY(check_pair(cQ, cP));
    if (cP) LR_TRY(same_stream(cQ, cP));
    std::unique_ptr<lr_refresh> h(new lr_refresh());
    LR_TRY(h->init(name, cQ, cP, max_batch, parsed));
    h->t = t;
    LR_HIP(hipSetDevice(cQ->device));
    const int nQ = h->nQ;
    const std::vector<u64> &q = cQ->h.q;
    // Recode's constants: q_m mod q_k, the Garner inverses, and per levelStart the digits of Q_ls >> 1 and Q_ls mod q_i
    std::vector<u64> tab((size_t)nQ * nQ + nQ + (size_t)2 * nQ * nQ, 0);
    u64 *qmod = tab.data(), *ginv = qmod + (size_t)nQ * nQ, *per = ginv + nQ;
    std::memset(&h->two64, 0, sizeof h->two64);
    Big Qls(1, 1);
    h->words.resize(nQ);
    for (int k = 0; k < nQ; ++k) {
        u64 prod = 1 % q[k];
        for (int m = 0; m < nQ; ++m) qmod[(size_t)k * nQ + m] = q[m] % q[k];
        for (int m = 0; m < k; ++m) prod = mulmod(prod, q[m] % q[k], q[k]);
        ginv[k] = k ? invmod(prod, q[k]) : 1;
        h->two64.v[k] = (u64)((((u128)1) << 64) % q[k]);
        big_mul(Qls, q[k]);                                       // Q_k, as :48-51 and :116-119 build it
        h->words[k] = (big_bitlen(Qls) + 63) / 64;
        u64 *hdig = per + (size_t)k * 2 * nQ, *qls = hdig + nQ;
        Big H = Qls;
        big_shr1(H);                                              // QHalf (:121)
        for (int m = 0; m <= k; ++m) hdig[m] = big_divmod(H, q[m]);
        for (int i = 0; i < nQ; ++i) {
            u64 r = 1 % q[i];
            for (int m = 0; m <= k; ++m) r = mulmod(r, q[m] % q[i], q[i]);
            qls[i] = r;
        }
    }
    const size_t N = (size_t)cQ->h.N, poly_words = (size_t)h->rows() * N;
    const size_t mask_words = std::max<size_t>(1, (size_t)std::min(h->words[nQ - 1], kCkksCrtMaxWords));
    LR_TRY(h->allocate((size_t)max_batch * (mask_words * N * sizeof(u64) + 2 * N)));
    LR_TRY(to_device(&h->d_tab, tab.data(), tab.size()));
    LR_HIP(hipMalloc((void **)&h->d_pool, (size_t)3 * max_batch * poly_words * sizeof(u64)));
    if (cP) LR_TRY(lr_bext_create(cQ, cP, &h->bext));
    if (t) {
        LR_TRY(lr_simple_scaler_create(cQ, t, &h->scaler));
        const std::vector<u64> delta = build_lift_params(cQ->h, t);
        LR_TRY(to_device(&h->d_delta, delta.data(), delta.size()));
        LR_HIP(hipMalloc((void **)&h->d_row, (size_t)max_batch * N * sizeof(u64)));
    }
    LR_HIP(hipStreamSynchronize(cQ->stream));          // the contexts may be given another stream before the first call
    *out = h.release();
    return LR_OK;
    });
}

extern "C" int lr_refresh_destroy(lr_refresh *h) {
    return guarded([&]() -> int { return destroy_handle(h); });
}

extern "C" int lr_refresh_mask_words(const lr_refresh *h, int level_start, int *words) {
    return guarded([&]() -> int {
    if (!h || !words) return fail(LR_ERR_ARG, "null argument");
    if (level_start < 0 || level_start + 1 > h->nQ) return h->refuse(LR_ERR_SHAPE, "level out of range");
    *words = h->words[level_start];
    return check_words(h, level_start);
    });
}

typedef const unsigned char *bytes_t;

extern "C" int lr_refresh_ckks_shares(lr_refresh *h, int level_start, const lr_poly *sk, const lr_poly *c1, const lr_poly *crs, const uint64_t *mask,
                                      const uint8_t *e0, const uint8_t *e1, int batch, lr_poly *share_decrypt, lr_poly *share_recrypt) {
    return guarded([&]() -> int { return ckks_shares(h, level_start, sk, c1, crs, mask, e0, e1, batch, share_decrypt, share_recrypt, false); });
}
extern "C" int lr_refresh_ckks_shares_device(lr_refresh *h, int level_start, const lr_poly *sk, const lr_poly *c1, const lr_poly *crs, const void *mask,
                                             const void *e0, const void *e1, int batch, lr_poly *share_decrypt, lr_poly *share_recrypt) {
    return guarded([&]() -> int {
        return ckks_shares(h, level_start, sk, c1, crs, (const u64 *)mask, (bytes_t)e0, (bytes_t)e1, batch, share_decrypt, share_recrypt, true);
    });
}
extern "C" int lr_refresh_ckks_recode(lr_refresh *h, int level_start, const lr_poly *in, lr_poly *out) {
    return guarded([&]() -> int { return ckks_recode(h, level_start, in, out); });
}
extern "C" int lr_refresh_ckks_finalize(lr_refresh *h, int level_start, const lr_poly *c0, const lr_poly *share_decrypt, const lr_poly *share_recrypt,
                                        lr_poly *out0) {
    return guarded([&]() -> int { return ckks_finalize(h, level_start, c0, share_decrypt, share_recrypt, out0); });
}
extern "C" int lr_refresh_bfv_shares(lr_refresh *h, const lr_poly *sk, const lr_poly *c1, const lr_poly *crs, const uint64_t *mask, const uint8_t *e0,
                                     const uint8_t *e1, int batch, lr_poly *share_decrypt, lr_poly *share_recrypt) {
    return guarded([&]() -> int { return bfv_shares(h, sk, c1, crs, mask, e0, e1, batch, share_decrypt, share_recrypt, false); });
}
extern "C" int lr_refresh_bfv_shares_device(lr_refresh *h, const lr_poly *sk, const lr_poly *c1, const lr_poly *crs, const void *mask, const void *e0,
                                            const void *e1, int batch, lr_poly *share_decrypt, lr_poly *share_recrypt) {
    return guarded([&]() -> int {
        return bfv_shares(h, sk, c1, crs, (const u64 *)mask, (bytes_t)e0, (bytes_t)e1, batch, share_decrypt, share_recrypt, true);
    });
}
extern "C" int lr_refresh_bfv_finalize(lr_refresh *h, const lr_poly *c0, const lr_poly *crs, const lr_poly *share_decrypt, const lr_poly *share_recrypt,
                                       lr_poly *out0, lr_poly *out1) {
    return guarded([&]() -> int { return bfv_finalize(h, c0, crs, share_decrypt, share_recrypt, out0, out1); });
}
extern "C" int lr_refresh_aggregate(lr_refresh *h, int level, const lr_poly *const *shares, int n_shares, lr_poly *out) {
    return guarded([&]() -> int { return fold_shares(h, h ? h->d_pool : nullptr, level, nullptr, shares, n_shares, out); });
}
