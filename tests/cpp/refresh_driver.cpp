// The Refresh handle's host side under AddressSanitizer + UBSan and under ThreadSanitizer (tests/test_host_refresh_sanitizers.py): the REAL
// host code -- lr_refresh.cpp with every other host unit of the library -- compiled with g++ against the host-only HIP stand-in and the
// launch stand-ins of tests/cpp/hipstub/, which touch the first and the last byte of everything a kernel would read or write.  Every entry
// point in its host and device-pointer form, both shapes (lr_options::no_epilogue), batches 1, 3 and max_batch with the pool and the
// staging buffer reused across consecutive host-form calls, wide polys, shared and per-ciphertext keys, every levelStart, ctxP present (|P|
// = 1, 2) and absent, 33 shares (a second fold pass) with out aliasing a share; two handles on two threads; every refusal.
// Exit code 0 = every check held; a sanitizer report aborts the run.  Nothing here computes: parity is the GPU suite's business.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#define REFUSED REFUSED_MSG      // here a refusal is logged with its message
#include "driver_check.hpp"

static const uint64_t T = 65537;
static const int MAXB = 5, SHARES = 33;

// one handle through every entry point (np = 0: the CKKS entry points only); returns the number of accepted calls
static int exercise(uint64_t N, int nq, int np, const lr_options *opt) {
    Rings r(N, Qm, nq, np, opt);
    const int rows = nq + np;
    lr_refresh *h = nullptr;
    OK(opt ? lr_refresh_create_ex(r.q, r.p, np ? T : 0, MAXB, opt, &h) : lr_refresh_create(r.q, r.p, np ? T : 0, MAXB, &h));
    if (!h) return 0;
    int calls = 0;
    for (int round = 0; round < 2; ++round)                                   // the second round reuses the pool and the staging buffer
        for (int n : {1, 3, MAXB}) {
            const bool wide = (n + round) % 2 == 1;                           // polys with one limb more than needed: another stride
            const int kb = round == 0 ? 1 : n;                                // the key: one for the call, or one per ciphertext
            for (int ls = 0; ls < nq; ++ls) {                                 // every levelStart
                int W = 0;
                OK(lr_refresh_mask_words(h, ls, &W));
                CHECK(W >= 1 && W <= 3);
                lr_poly *sk = poly(r.q, rows + (wide ? 1 : 0), kb), *c1 = poly(r.q, ls + 1 + (wide ? 1 : 0), n), *crs = poly(r.q, nq, n);
                lr_poly *dec = poly(r.q, ls + 1, n), *rec = poly(r.q, nq + (wide ? 1 : 0), n), *out = poly(r.q, nq, n), *c0 = poly(r.q, ls + 1, n);
                // exactly [n][W][N] words and [n][N] bytes
                std::vector<uint64_t> mask((size_t)n * W * N, ~0ull);
                std::vector<uint8_t> e((size_t)n * N, 0x93);
                void *dmask = nullptr, *de = nullptr;
                CHECK(hipMalloc(&dmask, mask.size() * sizeof(uint64_t)) == hipSuccess && hipMalloc(&de, e.size()) == hipSuccess);
                OK(lr_refresh_ckks_shares(h, ls, sk, c1, crs, mask.data(), e.data(), e.data(), n, dec, rec));
                OK(lr_refresh_ckks_shares(h, ls, sk, c1, crs, mask.data(), e.data(), e.data(), n, dec, rec));   // refills the pinned buffer
                OK(lr_refresh_ckks_shares_device(h, ls, sk, c1, crs, dmask, de, de, n, dec, rec));
                OK(lr_refresh_ckks_recode(h, ls, c0, out));
                OK(lr_refresh_ckks_recode(h, ls, out, out));                                            // in place
                OK(lr_refresh_ckks_finalize(h, ls, c0, dec, rec, out));
                calls += 6;
                OK(lr_context_sync(r.q));
                for (void *p : {dmask, de}) (void)hipFree(p);
                for (lr_poly *p : {sk, c1, crs, dec, rec, out, c0}) lr_poly_free(p);
            }
            if (np) {
                lr_poly *sk = poly(r.q, rows, kb), *c1 = poly(r.q, nq + (wide ? 1 : 0), n), *crs = poly(r.q, rows + (wide ? 1 : 0), n);
                lr_poly *dec = poly(r.q, nq, n), *rec = poly(r.q, nq + (wide ? 1 : 0), n), *o0 = poly(r.q, nq, n), *o1 = poly(r.q, nq, n), *c0 = poly(r.q, nq, n);
                std::vector<uint64_t> mask((size_t)n * N, T - 1);
                std::vector<uint8_t> e((size_t)n * N, 0x13);
                void *dmask = nullptr, *de = nullptr;
                CHECK(hipMalloc(&dmask, mask.size() * sizeof(uint64_t)) == hipSuccess && hipMalloc(&de, e.size()) == hipSuccess);
                OK(lr_refresh_bfv_shares(h, sk, c1, crs, mask.data(), e.data(), e.data(), n, dec, rec));
                OK(lr_refresh_bfv_shares_device(h, sk, c1, crs, dmask, de, de, n, dec, rec));
                OK(lr_refresh_bfv_finalize(h, c0, crs, dec, rec, o0, o1));
                OK(lr_refresh_bfv_finalize(h, c0, crs, dec, rec, c0, o1));                              // out0 = c0
                calls += 4;
                OK(lr_context_sync(r.q));
                for (void *p : {dmask, de}) (void)hipFree(p);
                for (lr_poly *p : {sk, c1, crs, dec, rec, o0, o1, c0}) lr_poly_free(p);
            }
            std::vector<lr_poly *> shares;
            for (int k = 0; k < SHARES; ++k) shares.push_back(poly(r.q, nq + (k % 2), n));
            lr_poly *out = poly(r.q, nq, n);
            const int level = (n + round) % nq;
            OK(lr_refresh_aggregate(h, level, shares.data(), 1, out));
            OK(lr_refresh_aggregate(h, level, shares.data(), 2, out));
            OK(lr_refresh_aggregate(h, level, shares.data(), SHARES, out));                             // two passes
            OK(lr_refresh_aggregate(h, level, shares.data(), SHARES, shares[SHARES - 1]));              // out = a share of the second pass
            calls += 4;
            OK(lr_context_sync(r.q));
            lr_poly_free(out);
            for (lr_poly *p : shares) lr_poly_free(p);
        }
    OK(lr_refresh_destroy(h));
    return calls;
}

static int refusals() {
    const uint64_t N = 16;
    const int nq = 3, np = 1, rows = 4, top = 2;
    int count = 0;
    Rings r(N, Qm, nq, np, nullptr), other(N, Qm, nq, np, nullptr);
    lr_context *small = nullptr, *big = nullptr, *dev1 = nullptr;
    OK(lr_context_create(4, Qm, nq, 0, &small));
    OK(lr_context_create(2 * N, Qm + nq, np, 0, &big));
    OK(lr_context_create(N, Qm + nq, np, 1, &dev1));
    lr_refresh *h = nullptr, *none = nullptr, *ckks_only = nullptr, *no_t = nullptr;
    // creation
    REFUSED(lr_refresh_create(nullptr, r.p, T, 1, &none) == LR_ERR_ARG);
    REFUSED(lr_refresh_create(r.q, r.p, T, 1, nullptr) == LR_ERR_ARG);
    REFUSED(lr_refresh_create(r.q, r.p, T, 0, &none) == LR_ERR_ARG && none == nullptr);
    REFUSED(lr_refresh_create(r.q, r.p, T, 65536, &none) == LR_ERR_ARG);
    REFUSED(lr_refresh_create(small, nullptr, 0, 1, &none) == LR_ERR_ARG);               // N < 8
    REFUSED(lr_refresh_create(r.q, big, T, 1, &none) == LR_ERR_ARG);                     // ctxP with another N
    REFUSED(lr_refresh_create(r.q, dev1, T, 1, &none) == LR_ERR_ARG);                    // ctxP on another device
    lr_options bad;
    OK(lr_options_init(&bad));
    bad.version = 99;
    REFUSED(lr_refresh_create_ex(r.q, r.p, T, 1, &bad, &none) == LR_ERR_ARG);
    {   // 64 limbs of Q and one of P: more rows than Q||P may hold; without the ctxP the same ring makes a handle
        lr_context *wide = nullptr;
        lr_refresh *fits = nullptr;
        OK(lr_context_create(N, Q64, 64, 0, &wide));
        REFUSED(lr_refresh_create(wide, r.p, T, 1, &none) == LR_ERR_UNSUPPORTED && none == nullptr);
        OK(lr_refresh_create(wide, nullptr, 0, 1, &fits));
        OK(lr_refresh_destroy(fits));
        OK(lr_context_destroy(wide));
    }
    count += 9;
    OK(lr_refresh_create(r.q, r.p, T, 2, &h));
    OK(lr_refresh_create(r.q, nullptr, 0, 2, &ckks_only));
    OK(lr_refresh_create(r.q, r.p, 0, 2, &no_t));
    lr_poly *sk = poly(r.q, rows, 1), *sk3 = poly(r.q, rows, 3), *skq = poly(r.q, nq, 1), *c1 = poly(r.q, nq, 2), *c11 = poly(r.q, nq, 1), *c13 = poly(r.q, nq, 3);
    lr_poly *crs = poly(r.q, rows, 2), *crsq = poly(r.q, nq, 2), *crs1 = poly(r.q, rows, 1), *crs3 = poly(r.q, rows, 3);
    lr_poly *dec = poly(r.q, nq, 2), *rec = poly(r.q, nq, 2), *o0 = poly(r.q, nq, 2), *o1 = poly(r.q, nq, 2), *o3 = poly(r.q, nq, 3), *d3 = poly(r.q, nq, 3);
    lr_poly *foreign = poly(other.q, nq, 2), *foreign1 = poly(other.q, rows, 1), *foreignc = poly(other.q, rows, 2), *narrow = poly(r.q, nq - 1, 2);
    lr_poly *s0 = poly(r.q, nq, 2), *s1 = poly(r.q, nq, 2), *s11 = poly(r.q, nq, 1);
    lr_poly *head = nullptr, *inside = nullptr;
    {
        uint64_t *d = nullptr;
        OK(lr_poly_info(o0, nullptr, nullptr, nullptr, (void **)&d));
        OK(lr_poly_wrap(r.q, d, nq, 1, &head));                                         // member 0 of o0
        OK(lr_poly_wrap(r.q, d + N, nq, 1, &inside));                                   // from limb 1 of member 0 on: a partial overlap with head
    }
    const lr_poly *two[2] = {s0, s1}, *with_null[2] = {s0, nullptr}, *with_foreign[2] = {s0, foreign}, *mixed[2] = {s0, s11}, *one3[1] = {o3},
                  *one_inside[1] = {inside};
    std::vector<uint64_t> words((size_t)3 * 3 * N, 0);
    const uint64_t *m = words.data();
    const uint8_t *u = (const uint8_t *)words.data();
    int W = 0;
    // NULL arguments
    REFUSED(lr_refresh_mask_words(nullptr, 0, &W) == LR_ERR_ARG);
    REFUSED(lr_refresh_mask_words(h, 0, nullptr) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_shares(nullptr, top, sk, c1, crsq, m, u, u, 2, dec, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_shares(h, top, nullptr, c1, crsq, m, u, u, 2, dec, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_shares_device(h, top, sk, nullptr, crsq, m, u, u, 2, dec, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_shares(h, top, sk, c1, nullptr, m, u, u, 2, dec, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_shares_device(h, top, sk, c1, crsq, nullptr, u, u, 2, dec, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_shares(h, top, sk, c1, crsq, m, nullptr, u, 2, dec, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_shares(h, top, sk, c1, crsq, m, u, nullptr, 2, dec, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_shares(h, top, sk, c1, crsq, m, u, u, 2, nullptr, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_shares(h, top, sk, c1, crsq, m, u, u, 2, dec, nullptr) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_recode(nullptr, top, c1, o0) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_recode(h, top, nullptr, o0) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_recode(h, top, c1, nullptr) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_finalize(nullptr, top, c1, dec, rec, o0) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_finalize(h, top, nullptr, dec, rec, o0) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_finalize(h, top, c1, nullptr, rec, o0) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_finalize(h, top, c1, dec, nullptr, o0) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_finalize(h, top, c1, dec, rec, nullptr) == LR_ERR_ARG);
    REFUSED(lr_refresh_bfv_shares(nullptr, sk, c1, crs, m, u, u, 2, dec, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_bfv_shares(h, nullptr, c1, crs, m, u, u, 2, dec, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_bfv_shares_device(h, sk, c1, nullptr, m, u, u, 2, dec, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_bfv_shares_device(h, sk, c1, crs, nullptr, u, u, 2, dec, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_bfv_shares(h, sk, c1, crs, m, u, u, 2, dec, nullptr) == LR_ERR_ARG);
    REFUSED(lr_refresh_bfv_finalize(nullptr, c1, crs, dec, rec, o0, o1) == LR_ERR_ARG);
    REFUSED(lr_refresh_bfv_finalize(h, c1, nullptr, dec, rec, o0, o1) == LR_ERR_ARG);
    REFUSED(lr_refresh_bfv_finalize(h, c1, crs, dec, rec, o0, nullptr) == LR_ERR_ARG);
    REFUSED(lr_refresh_aggregate(nullptr, top, two, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_refresh_aggregate(h, top, nullptr, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_refresh_aggregate(h, top, with_null, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_refresh_aggregate(h, top, two, 2, nullptr) == LR_ERR_ARG);
    count += 31;
    // a poly of another context, an output that shares memory with an input or with the other output, a partial overlap, alignment
    REFUSED(lr_refresh_ckks_shares(h, top, foreign1, c1, crsq, m, u, u, 2, dec, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_shares(h, top, sk, foreign, crsq, m, u, u, 2, dec, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_shares(h, top, sk, c1, foreign, m, u, u, 2, dec, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_shares(h, top, sk, c1, crsq, m, u, u, 2, dec, foreign) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_shares(h, top, sk, c1, crsq, m, u, u, 2, c1, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_shares(h, top, sk, c1, crsq, m, u, u, 2, dec, crsq) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_shares(h, top, sk, c1, crsq, m, u, u, 2, dec, dec) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_shares_device(h, top, sk, c1, crsq, u + 4, u, u, 2, dec, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_bfv_shares(h, sk, c1, foreignc, m, u, u, 2, dec, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_bfv_shares(h, sk, c1, crs, m, u, u, 2, foreign, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_bfv_shares(h, sk, c1, crs, m, u, u, 2, dec, c1) == LR_ERR_ARG);
    REFUSED(lr_refresh_bfv_shares(h, sk, c11, crs1, m, u, u, 1, head, inside) == LR_ERR_ARG);
    REFUSED(lr_refresh_bfv_shares_device(h, sk, c1, crs, u + 8, u, u, 2, dec, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_recode(h, top, foreign, o0) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_recode(h, top, c1, foreign) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_recode(h, top, inside, head) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_finalize(h, top, foreign, dec, rec, o0) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_finalize(h, top, c1, dec, rec, dec) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_finalize(h, top, c1, dec, rec, rec) == LR_ERR_ARG);
    REFUSED(lr_refresh_ckks_finalize(h, top, inside, s11, c11, head) == LR_ERR_ARG);             // out0 overlaps c0 without being it
    REFUSED(lr_refresh_bfv_finalize(h, c1, crs, dec, rec, o0, foreign) == LR_ERR_ARG);
    REFUSED(lr_refresh_bfv_finalize(h, c1, crs, dec, rec, o0, o0) == LR_ERR_ARG);
    REFUSED(lr_refresh_bfv_finalize(h, c1, crs, dec, rec, o0, c1) == LR_ERR_ARG);                // only out0 may be c0
    REFUSED(lr_refresh_bfv_finalize(h, c1, crs, dec, rec, dec, o1) == LR_ERR_ARG);
    REFUSED(lr_refresh_aggregate(h, top, with_foreign, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_refresh_aggregate(h, top, two, 2, foreign) == LR_ERR_ARG);
    REFUSED(lr_refresh_aggregate(h, top, one_inside, 1, head) == LR_ERR_ARG);
    count += 27;
    // a handle without P or without t: the CKKS entry points only
    for (lr_refresh *hc : {ckks_only, no_t}) {
        REFUSED(lr_refresh_bfv_shares(hc, sk, c1, crs, m, u, u, 2, dec, rec) == LR_ERR_ARG);
        CHECK(std::string(lr_last_error_string()).find("CKKS entry points only") != std::string::npos);
        REFUSED(lr_refresh_bfv_finalize(hc, c1, crs, dec, rec, o0, o1) == LR_ERR_ARG);
        OK(lr_refresh_ckks_shares(hc, top, skq, c1, crsq, m, u, u, 2, dec, rec));
        count += 2;
    }
    // levels, batches and limbs
    REFUSED(lr_refresh_mask_words(h, nq, &W) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_mask_words(h, -1, &W) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_ckks_shares(h, nq, sk, c1, crsq, m, u, u, 2, dec, rec) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_ckks_shares(h, -1, sk, c1, crsq, m, u, u, 2, dec, rec) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_ckks_shares(h, top, sk, c1, crsq, m, u, u, 0, dec, rec) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_ckks_shares(h, top, sk3, c13, crs3, m, u, u, 3, d3, o3) == LR_ERR_SHAPE);     // above max_batch
    REFUSED(lr_refresh_ckks_shares(h, top, sk, c1, crsq, m, u, u, 1, dec, rec) == LR_ERR_SHAPE);     // differs from the polys'
    REFUSED(lr_refresh_ckks_shares(h, top, sk3, c1, crsq, m, u, u, 2, dec, rec) == LR_ERR_SHAPE);    // the key: batch 1 or the call's
    REFUSED(lr_refresh_ckks_shares(h, top, sk, c11, crsq, m, u, u, 2, dec, rec) == LR_ERR_SHAPE);    // c1 of batch 1
    REFUSED(lr_refresh_ckks_shares(h, top, sk, c1, crs1, m, u, u, 2, dec, rec) == LR_ERR_SHAPE);     // crs of batch 1
    REFUSED(lr_refresh_ckks_shares(h, top, sk, narrow, crsq, m, u, u, 2, dec, rec) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_ckks_shares(h, top - 1, sk, narrow, crsq, m, u, u, 2, dec, narrow) == LR_ERR_SHAPE);   // share_recrypt is over all of Q
    OK(lr_refresh_ckks_shares(h, top - 1, sk, narrow, crsq, m, u, u, 2, dec, rec));                  // ... and c1 is wide enough one level down
    REFUSED(lr_refresh_bfv_shares(h, skq, c1, crs, m, u, u, 2, dec, rec) == LR_ERR_SHAPE);           // sk without the rows of P
    REFUSED(lr_refresh_bfv_shares(h, sk, c1, crsq, m, u, u, 2, dec, rec) == LR_ERR_SHAPE);           // crs without the rows of P
    REFUSED(lr_refresh_bfv_shares(h, sk, narrow, crs, m, u, u, 2, dec, rec) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_bfv_shares(h, sk, c1, crs, m, u, u, -1, dec, rec) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_ckks_recode(h, nq, c1, o0) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_ckks_recode(h, top, narrow, o0) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_ckks_recode(h, 0, c1, narrow) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_ckks_recode(h, top, c11, o0) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_ckks_recode(h, top, c13, o3) == LR_ERR_SHAPE);                                // above max_batch
    REFUSED(lr_refresh_ckks_finalize(h, nq, c1, dec, rec, o0) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_ckks_finalize(h, 0, c1, dec, narrow, o0) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_ckks_finalize(h, top, c1, dec, s11, o0) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_bfv_finalize(h, c1, crsq, dec, rec, o0, o1) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_bfv_finalize(h, c1, crs, dec, rec, o0, s11) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_bfv_finalize(h, narrow, crs, dec, rec, o0, o1) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_aggregate(h, top, two, 0, o0) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_aggregate(h, nq, two, 2, o0) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_aggregate(h, top, mixed, 2, o0) == LR_ERR_SHAPE);                             // every poly has the same batch
    REFUSED(lr_refresh_aggregate(h, top, two, 2, narrow) == LR_ERR_SHAPE);
    REFUSED(lr_refresh_aggregate(h, top, one3, 1, o3) == LR_ERR_SHAPE);                              // above max_batch
    count += 32;
    {   // the two contexts on different streams: every entry point refuses, and so does creation
        hipStream_t st = nullptr;
        CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
        OK(lr_context_set_stream(r.q, st));
        REFUSED(lr_refresh_ckks_shares(h, top, sk, c1, crsq, m, u, u, 2, dec, rec) == LR_ERR_ARG);
        CHECK(std::string(lr_last_error_string()).find("different streams") != std::string::npos);
        REFUSED(lr_refresh_bfv_shares_device(h, sk, c1, crs, m, u, u, 2, dec, rec) == LR_ERR_ARG);
        REFUSED(lr_refresh_ckks_recode(h, top, c1, o0) == LR_ERR_ARG);
        REFUSED(lr_refresh_ckks_finalize(h, top, c1, dec, rec, o0) == LR_ERR_ARG);
        REFUSED(lr_refresh_bfv_finalize(h, c1, crs, dec, rec, o0, o1) == LR_ERR_ARG);
        REFUSED(lr_refresh_aggregate(h, top, two, 2, o0) == LR_ERR_ARG);
        REFUSED(lr_refresh_create(r.q, r.p, T, 1, &none) == LR_ERR_ARG && none == nullptr);
        OK(lr_refresh_ckks_recode(ckks_only, top, c1, o0));                                          // (a handle without a ctxP has one stream)
        OK(lr_context_sync(r.q));
        OK(lr_context_set_stream(r.q, nullptr));
        CHECK(hipStreamDestroy(st) == hipSuccess);
        count += 7;
    }
    OK(lr_refresh_aggregate(h, top, two, 2, s0));                                        // the handle stays usable
    for (lr_poly *p : {sk, sk3, skq, c1, c11, c13, crs, crsq, crs1, crs3, dec, rec, o0, o1, o3, d3, foreign, foreign1, foreignc, narrow, s0, s1, s11, head, inside})
        lr_poly_free(p);
    OK(lr_refresh_destroy(no_t));
    OK(lr_refresh_destroy(ckks_only));
    OK(lr_refresh_destroy(h));
    OK(lr_refresh_destroy(nullptr));
    OK(lr_context_destroy(dev1));
    OK(lr_context_destroy(big));
    OK(lr_context_destroy(small));
    return count;
}

int main() {
    int calls = 0, refused = 0;
    lr_options call_by_call;
    OK(lr_options_init(&call_by_call));
    call_by_call.no_epilogue = 1;
    for (uint64_t N : {(uint64_t)1 << 4, (uint64_t)1 << 12}) {
        calls += exercise(N, 3, 1, nullptr);
        calls += exercise(N, 3, 2, &call_by_call);
    }
    calls += exercise(1 << 4, 3, 2, nullptr);
    calls += exercise(1 << 4, 3, 1, &call_by_call);
    calls += exercise(1 << 4, 3, 0, nullptr);                                            // ctxP absent
    calls += exercise(1 << 4, 3, 0, &call_by_call);
    refused += refusals();
    {   // two handles on two threads, each with its own contexts: nothing is shared but the library's globals
        std::atomic<int> threaded{0};
        std::thread a([&] { threaded += exercise(1 << 12, 3, 2, nullptr); });
        std::thread b([&] { threaded += exercise(1 << 4, 3, 1, &call_by_call); });
        a.join();
        b.join();
        calls += threaded.load();
    }
    return driver_end(ALLOCATIONS | EVENTS | LOG, refused, "refresh: calls %d, refusals %d", calls, refused);
}
