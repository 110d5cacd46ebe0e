// The collective setup's host side under AddressSanitizer + UBSan and under ThreadSanitizer (tests/test_host_setup_sanitizers.py): the REAL
// host code -- lr_setup.cpp with every other host unit of the library -- compiled with g++ against the host-only HIP stand-in and the
// launch stand-ins of tests/cpp/hipstub/, which touch the first and the last byte of everything a kernel would read or write.  Every entry
// point in its host and device-pointer form, both shapes (lr_options::no_epilogue), 1, 3 and max_batch parties (5, and 70: more than one
// pass) with the pool and the staging buffer reused across consecutive host-form calls, wide polys, shared and per-party keys, |P| = 1 and
// a ragged |P| = 2 whose last digit owns one row; two handles on two threads; the launch counts of both shapes; every refusal a context can
// be made for (N > 2^30 has none: include/lattigo_ring.h).
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

namespace lr {
extern std::atomic<unsigned long long> g_stub_launches, g_ckks_expand_launches, g_fold_launches, g_setup_ckg_launches, g_setup_share_launches,
    g_setup_key_launches;
}  // namespace lr

static const int MAXB = 5;
static const int ENTRY_POINTS = 20;      // accepted calls per party count in exercise(): 14 share calls, 3 finalize steps, 3 folds

// one handle through every entry point; returns the number of accepted calls.  max_n above kSetupPartiesPerLaunch (32): a call runs as
// several passes over the pool, each with its own offsets into the bytes, the keys, the Galois elements and the share array
static int exercise(uint64_t N, int nq, int np, const lr_options *opt, int max_n = MAXB) {
    Rings r(N, Qm, nq, np, opt);
    const int rows = nq + np, beta = (nq + np - 1) / np;
    lr_setup *s = nullptr;
    OK(opt ? lr_setup_create_ex(r.q, r.p, max_n, opt, &s) : lr_setup_create(r.q, r.p, max_n, &s));
    if (!s) return 0;
    int calls = 0;
    for (int round = 0; round < 2; ++round)                                   // the second round reuses the pool and the staging buffer
        for (int n : {1, 3, max_n}) {
            const bool wide = (n + round) % 2 == 1;                           // polys with one limb more than needed: another stride
            const int kb = round == 0 ? 1 : n, w = wide ? 1 : 0;              // keys: one for the call, or one per party
            lr_poly *sk = poly(r.q, rows + w, kb), *u = poly(r.q, rows + 1 - w, kb), *sk1 = poly(r.q, rows, 1), *crs = poly(r.q, rows + w, 1);
            lr_poly *crp = poly(r.q, rows + 1 - w, beta), *pk0 = poly(r.q, rows, 1), *pk1 = poly(r.q, rows + w, 1), *ckg = poly(r.q, rows + w, n);
            lr_poly *r1 = poly(r.q, rows + w, beta), *r2 = poly(r.q, rows + 1 - w, 2 * beta), *r3 = poly(r.q, rows, beta);
            lr_poly *evk = poly(r.q, rows + w, 2 * beta);
            std::vector<lr_poly *> polys, pairs;
            for (int k = 0; k < n; ++k) {
                polys.push_back(poly(r.q, rows + ((k + w) % 2), beta));
                pairs.push_back(poly(r.q, rows + ((k + 1 + w) % 2), 2 * beta));
            }
            // exactly [n][N], [n][beta][N], [n][beta][2][N] and [n][beta][N / 8] bytes
            std::vector<uint8_t> e0((size_t)n * N, 0x93), e1((size_t)n * beta * N, 0x80), e2((size_t)n * beta * 2 * N, 0x13),
                bits((size_t)n * beta * N / 8, 0xAA);
            std::vector<uint64_t> gens;
            for (int k = 0; k < n; ++k) gens.push_back(k % 3 == 0 ? 5 : (k % 3 == 1 ? 2 * N - 1 : 1));
            void *de0 = nullptr, *de1 = nullptr, *de2 = nullptr, *dbits = nullptr;
            CHECK(hipMalloc(&de0, e0.size()) == hipSuccess && hipMalloc(&de1, e1.size()) == hipSuccess && hipMalloc(&de2, e2.size()) == hipSuccess &&
                  hipMalloc(&dbits, bits.size()) == hipSuccess);
            // host-form calls one behind the other: each refills the pinned buffer the one before staged through
            OK(lr_setup_ckg_share(s, sk, crs, e0.data(), n, ckg));
            OK(lr_setup_rkg_round1(s, u, sk, crp, e1.data(), n, polys.data()));
            OK(lr_setup_rkg_round2(s, r1, sk, crp, e2.data(), n, pairs.data()));
            OK(lr_setup_rkg_round3(s, r2, u, sk, e1.data(), n, polys.data()));
            OK(lr_setup_rkg_naive_round1(s, round ? LR_SETUP_CKKS : LR_SETUP_BFV, sk, pk0, pk1, e2.data(), bits.data(), bits.data(), n, pairs.data()));
            OK(lr_setup_rkg_naive_round2(s, r2, sk, pk0, pk1, bits.data(), bits.data(), e2.data(), n, pairs.data()));
            OK(lr_setup_rtg_share(s, sk1, gens.data(), n, crp, e1.data(), polys.data()));
            OK(lr_setup_ckg_share_device(s, sk, crs, de0, n, ckg));
            OK(lr_setup_rkg_round1_device(s, u, sk, crp, de1, n, polys.data()));
            OK(lr_setup_rkg_round2_device(s, r1, sk, crp, de2, n, pairs.data()));
            OK(lr_setup_rkg_round3_device(s, r2, u, sk, de1, n, polys.data()));
            OK(lr_setup_rkg_naive_round1_device(s, round ? LR_SETUP_BFV : LR_SETUP_CKKS, sk, pk0, pk1, de2, dbits, dbits, n, pairs.data()));
            OK(lr_setup_rkg_naive_round2_device(s, r2, sk, pk0, pk1, dbits, dbits, de2, n, pairs.data()));
            OK(lr_setup_rtg_share_device(s, sk1, gens.data(), n, crp, de1, polys.data()));
            // the finalize steps, fresh and in place, and the fold over shares of beta polys, of pairs and of one poly
            OK(lr_setup_rkg_key(s, r2, r3, round ? r2 : evk));
            OK(lr_setup_rkg_naive_key(s, pairs[0], round ? pairs[0] : evk));
            OK(lr_setup_rtg_key(s, r1, crp, evk));
            calls += ENTRY_POINTS;
            OK(lr_setup_aggregate(s, polys.data(), n, round ? polys[n - 1] : r1));
            OK(lr_setup_aggregate(s, pairs.data(), n, round ? pairs[0] : evk));
            {
                const lr_poly *ones[2] = {pk0, pk1};
                OK(lr_setup_aggregate(s, ones, 2, round ? pk1 : sk1));
            }
            OK(lr_context_sync(r.q));
            for (void *p : {de0, de1, de2, dbits}) (void)hipFree(p);
            for (lr_poly *p : {sk, u, sk1, crs, crp, pk0, pk1, ckg, r1, r2, r3, evk}) lr_poly_free(p);
            for (lr_poly *p : polys) lr_poly_free(p);
            for (lr_poly *p : pairs) lr_poly_free(p);
        }
    OK(lr_setup_destroy(s));
    return calls;
}

// at N = 2^4 a transform is one launch per context: the default shape of a share call is expansion, transform, share -- ONE launch each
// for all parties -- and the call-by-call shape the reference's Context calls per party and digit
static void sequences() {
    const uint64_t N = 16;
    const int nq = 3, np = 2, beta = 2, n = 3, rows = nq + np;
    for (int call_by_call : {0, 1}) {
        lr_options opt;
        OK(lr_options_init(&opt));
        opt.no_epilogue = call_by_call;
        Rings r(N, Qm, nq, np, &opt);
        lr_setup *s = nullptr;
        OK(lr_setup_create_ex(r.q, r.p, n, &opt, &s));
        lr_poly *sk = poly(r.q, rows, n), *u = poly(r.q, rows, n), *sk1 = poly(r.q, rows, 1), *crs = poly(r.q, rows, 1), *crp = poly(r.q, rows, beta);
        lr_poly *ckg = poly(r.q, rows, n), *r1 = poly(r.q, rows, beta), *r2 = poly(r.q, rows, 2 * beta), *evk = poly(r.q, rows, 2 * beta);
        std::vector<lr_poly *> polys, pairs;
        for (int k = 0; k < n; ++k) polys.push_back(poly(r.q, rows, beta)), pairs.push_back(poly(r.q, rows, 2 * beta));
        std::vector<uint8_t> e((size_t)n * beta * 2 * N, 0x80);
        const uint64_t gens[3] = {5, 2 * N - 1, 1};
        auto snap = [] {
            return std::vector<unsigned long long>{lr::g_stub_launches.load(),      lr::g_ckks_expand_launches.load(), lr::g_setup_ckg_launches.load(),
                                                   lr::g_setup_share_launches.load(), lr::g_setup_key_launches.load(),   lr::g_fold_launches.load()};
        };
        std::vector<unsigned long long> s0, d;
        auto diff = [&] {
            d = snap();
            for (size_t i = 0; i < d.size(); ++i) d[i] -= s0[i];
        };
        // d[0]: transforms and Context calls; d[1]: expansions; d[2], d[3], d[4], d[5]: the handle's own kernels and the fold
        const unsigned long long cc = call_by_call;
        s0 = snap();
        OK(lr_setup_ckg_share(s, sk, crs, e.data(), n, ckg));
        diff();      // MulCoeffsMontgomeryAndSub over Q and P
        CHECK(d[1] == 1 && d[2] == 1 - cc && d[0] == 2 + cc * 2);
        s0 = snap();
        OK(lr_setup_rkg_round1(s, u, sk, crp, e.data(), n, polys.data()));
        diff();      // per party MulScalarBigint, InvMForm; per digit the sampler's copy (Q, P), Add, MulCoeffsMontgomeryAndSub (Q, P)
        CHECK(d[1] == 1 && d[3] == 1 - cc && d[0] == 2 + cc * n * (2 + beta * 5));
        s0 = snap();
        OK(lr_setup_rkg_round2(s, r1, sk, crp, e.data(), n, pairs.data()));
        diff();      // per digit MulCoeffsMontgomery, Add, the sampler's copy, MulCoeffsMontgomeryAndAdd, each over Q and P
        CHECK(d[1] == 1 && d[3] == 1 - cc && d[0] == 2 + cc * n * beta * 8);
        s0 = snap();
        OK(lr_setup_rkg_round3(s, r2, u, sk, e.data(), n, polys.data()));
        diff();      // per party Sub; per digit the sampler's copy and MulCoeffsMontgomeryAndAdd
        CHECK(d[1] == 1 && d[3] == 1 - cc && d[0] == 2 + cc * n * (2 + beta * 4));
        s0 = snap();
        OK(lr_setup_rkg_key(s, r2, r1, evk));
        diff();      // per digit Add, Copy, MForm, MForm
        CHECK(d[1] == 0 && d[4] == 1 - cc && d[0] == cc * beta * 8);
        s0 = snap();
        OK(lr_setup_rkg_key(s, r2, r1, r2));
        diff();      // in place: no Copy
        CHECK(d[4] == 1 - cc && d[0] == cc * beta * 6);
        for (int scheme : {LR_SETUP_BFV, LR_SETUP_CKKS}) {
            s0 = snap();
            OK(lr_setup_rkg_naive_round1(s, scheme, sk, crs, sk1, e.data(), e.data(), e.data(), n, pairs.data()));
            diff();  // two expansions (noise, ternary); per party MulScalarBigint, InvMForm; per digit two copies, Add, two MulCoeffsMontgomeryAndAdd
            CHECK(d[1] == 2 && d[3] == 1 - cc && d[0] == 2 + cc * n * (2 + beta * 9));
        }
        s0 = snap();
        OK(lr_setup_rkg_naive_round2(s, r2, sk, crs, sk1, e.data(), e.data(), e.data(), n, pairs.data()));
        diff();      // per digit two MulCoeffsMontgomery, two MulCoeffsMontgomeryAndAdd, two Add
        CHECK(d[1] == 2 && d[3] == 1 - cc && d[0] == 2 + cc * n * beta * 12);
        s0 = snap();
        OK(lr_setup_rkg_naive_key(s, r2, evk));
        diff();
        CHECK(d[4] == 1 - cc && d[0] == cc * beta * 8);
        s0 = snap();
        OK(lr_setup_rtg_share(s, sk1, gens, n, crp, e.data(), polys.data()));
        diff();      // per key PermuteNTT (not for the element 1), MulScalarBigint, InvMForm; per digit copy, Add, MulCoeffsMontgomeryAndSub, MForm
        CHECK(d[1] == 1 && d[3] == 1 - cc && d[0] == 2 + cc * (n * 3 - 1 + n * beta * 7));
        s0 = snap();
        OK(lr_setup_rtg_key(s, r1, crp, evk));
        diff();
        CHECK(d[4] == 1 - cc && d[0] == cc * beta * 4);
        s0 = snap();
        OK(lr_setup_aggregate(s, polys.data(), n, r1));
        diff();      // n - 1 Context.Add over Q and P
        CHECK(d[5] == 1 - cc && d[0] == cc * (n - 1) * 2);
        for (lr_poly *p : {sk, u, sk1, crs, crp, ckg, r1, r2, evk}) lr_poly_free(p);
        for (lr_poly *p : polys) lr_poly_free(p);
        for (lr_poly *p : pairs) lr_poly_free(p);
        OK(lr_setup_destroy(s));
    }
}

static int refusals() {
    const uint64_t N = 16;
    const int nq = 3, np = 1, rows = 4, beta = 3;
    Rings r(N, Qm, nq, np, nullptr), other(N, Qm, nq, np, nullptr);
    lr_context *small = nullptr, *big = nullptr, *dev1 = nullptr;
    OK(lr_context_create(4, Qm, nq, 0, &small));
    OK(lr_context_create(2 * N, Qm + nq, np, 0, &big));
    OK(lr_context_create(N, Qm + nq, np, 1, &dev1));
    lr_setup *s = nullptr, *none = nullptr, *no_p = nullptr;
    const unsigned long long before = lr::g_stub_launches.load() + lr::g_ckks_expand_launches.load() + lr::g_fold_launches.load();
    // creation
    REFUSED(lr_setup_create(nullptr, r.p, 1, &none) == LR_ERR_ARG);
    REFUSED(lr_setup_create(r.q, r.p, 1, nullptr) == LR_ERR_ARG);
    REFUSED(lr_setup_create(r.q, r.p, 0, &none) == LR_ERR_ARG && none == nullptr);
    REFUSED(lr_setup_create(r.q, r.p, 65536, &none) == LR_ERR_ARG);
    REFUSED(lr_setup_create(small, nullptr, 1, &none) == LR_ERR_ARG);                 // N < 8
    REFUSED(lr_setup_create(r.q, big, 1, &none) == LR_ERR_ARG);                       // ctxP with another N
    REFUSED(lr_setup_create(r.q, dev1, 1, &none) == LR_ERR_ARG);                      // ctxP on another device
    lr_options bad;
    OK(lr_options_init(&bad));
    bad.version = 99;
    REFUSED(lr_setup_create_ex(r.q, r.p, 1, &bad, &none) == LR_ERR_ARG);
    {   // 64 limbs of Q and one of P: more rows than Q||P may hold; without the ctxP the same ring makes a handle (CKG over Q).  The other
        // LR_ERR_UNSUPPORTED of the header, N > 2^30, has no context to be tried with: see the header
        lr_context *wide = nullptr;
        lr_setup *fits = nullptr;
        OK(lr_context_create(N, Q64, 64, 0, &wide));
        REFUSED(lr_setup_create(wide, r.p, 1, &none) == LR_ERR_UNSUPPORTED && none == nullptr);
        OK(lr_setup_create(wide, nullptr, 1, &fits));
        OK(lr_setup_destroy(fits));
        OK(lr_context_destroy(wide));
    }
    OK(lr_setup_create(r.q, r.p, 2, &s));
    OK(lr_setup_create(r.q, nullptr, 2, &no_p));
    lr_poly *sk = poly(r.q, rows, 2), *u = poly(r.q, rows, 2), *sk1 = poly(r.q, rows, 1), *sk3 = poly(r.q, rows, 3), *crs = poly(r.q, rows, 1);
    lr_poly *crp = poly(r.q, rows, beta), *ckg = poly(r.q, rows, 2), *r1 = poly(r.q, rows, beta), *r2 = poly(r.q, rows, 2 * beta), *r3 = poly(r.q, rows, beta);
    lr_poly *evk = poly(r.q, rows, 2 * beta), *pk0 = poly(r.q, rows, 1), *pk1 = poly(r.q, rows, 1);
    lr_poly *foreign = poly(other.q, rows, 2), *foreign1 = poly(other.q, rows, 1), *fshare = poly(other.q, rows, beta), *fpair = poly(other.q, rows, 2 * beta);
    lr_poly *narrow = poly(r.q, rows - 1, 2), *nshare = poly(r.q, rows - 1, beta), *npair = poly(r.q, rows - 1, 2 * beta), *odd = poly(r.q, rows, 2 * beta + 1);
    lr_poly *a0 = poly(r.q, rows, beta), *a1 = poly(r.q, rows, beta), *a2 = poly(r.q, rows, beta);
    lr_poly *b0 = poly(r.q, rows, 2 * beta), *b1 = poly(r.q, rows, 2 * beta), *skq = poly(r.q, nq, 2), *crsq = poly(r.q, nq, 1), *ckgq = poly(r.q, nq, 2);
    lr_poly *inside = nullptr, *head = nullptr, *tail = nullptr;
    {
        uint64_t *d = nullptr;
        OK(lr_poly_info(a0, nullptr, nullptr, nullptr, (void **)&d));
        OK(lr_poly_wrap(r.q, d + (size_t)rows * N, rows, 1, &inside));                // member 1 of a0
        OK(lr_poly_info(odd, nullptr, nullptr, nullptr, (void **)&d));
        OK(lr_poly_wrap(r.q, d, rows, 2 * beta, &head));                              // members 0 .. 2 beta - 1 of odd ...
        OK(lr_poly_wrap(r.q, d + (size_t)rows * N, rows, 2 * beta, &tail));           // ... and members 1 .. 2 beta: a partial overlap
    }
    lr_poly *polys[2] = {a0, a1}, *pairs[2] = {b0, b1}, *same[2] = {a0, a0}, *with_null[2] = {a0, nullptr}, *with_foreign[2] = {a0, fshare},
            *with_narrow[2] = {a0, nshare}, *three[3] = {a0, a1, a2}, *one[1] = {a0};
    const lr_poly *mixed[2] = {r1, r2}, *shares[2] = {r1, r3}, *ones[2] = {pk0, pk1}, *overl[1] = {head};
    std::vector<uint8_t> b((size_t)3 * beta * 2 * N, 0);
    const uint8_t *e = b.data();
    const uint64_t g[3] = {5, 25, 125}, even[2] = {5, 6}, zero[2] = {0, 5};
    int count = 9;
#define R(x) do { REFUSED(x); ++count; } while (0)
    // a handle without P: CKG and its fold over Q, nothing else
    R(lr_setup_rkg_round1(no_p, u, sk, crp, e, 2, polys) == LR_ERR_ARG);
    CHECK(std::string(lr_last_error_string()).find("modulus P is empty") != std::string::npos);
    R(lr_setup_rkg_round2_device(no_p, r1, sk, crp, e, 2, pairs) == LR_ERR_ARG);
    R(lr_setup_rkg_round3(no_p, r2, u, sk, e, 2, polys) == LR_ERR_ARG);
    R(lr_setup_rkg_key(no_p, r2, r3, evk) == LR_ERR_ARG);
    R(lr_setup_rkg_naive_round1(no_p, LR_SETUP_BFV, sk, pk0, pk1, e, e, e, 2, pairs) == LR_ERR_ARG);
    R(lr_setup_rkg_naive_round2(no_p, r2, sk, pk0, pk1, e, e, e, 2, pairs) == LR_ERR_ARG);
    R(lr_setup_rkg_naive_key(no_p, r2, evk) == LR_ERR_ARG);
    R(lr_setup_rtg_share(no_p, sk1, g, 2, crp, e, polys) == LR_ERR_ARG);
    R(lr_setup_rtg_key(no_p, r1, crp, evk) == LR_ERR_ARG);
    R(lr_setup_aggregate(no_p, shares, 2, r1) == LR_ERR_SHAPE);                        // without P a poly has batch 1
    OK(lr_setup_ckg_share(no_p, skq, crsq, e, 2, ckgq));
    // NULL arguments
    R(lr_setup_ckg_share(nullptr, sk, crs, e, 2, ckg) == LR_ERR_ARG);
    R(lr_setup_ckg_share(s, nullptr, crs, e, 2, ckg) == LR_ERR_ARG);
    R(lr_setup_ckg_share(s, sk, nullptr, e, 2, ckg) == LR_ERR_ARG);
    R(lr_setup_ckg_share_device(s, sk, crs, nullptr, 2, ckg) == LR_ERR_ARG);
    R(lr_setup_ckg_share(s, sk, crs, e, 2, nullptr) == LR_ERR_ARG);
    R(lr_setup_rkg_round1(s, nullptr, sk, crp, e, 2, polys) == LR_ERR_ARG);
    R(lr_setup_rkg_round1(s, u, nullptr, crp, e, 2, polys) == LR_ERR_ARG);
    R(lr_setup_rkg_round1(s, u, sk, nullptr, e, 2, polys) == LR_ERR_ARG);
    R(lr_setup_rkg_round1_device(s, u, sk, crp, nullptr, 2, polys) == LR_ERR_ARG);
    R(lr_setup_rkg_round1(s, u, sk, crp, e, 2, nullptr) == LR_ERR_ARG);
    R(lr_setup_rkg_round1(s, u, sk, crp, e, 2, with_null) == LR_ERR_ARG);
    R(lr_setup_rkg_round2(s, nullptr, sk, crp, e, 2, pairs) == LR_ERR_ARG);
    R(lr_setup_rkg_round2_device(s, r1, sk, crp, nullptr, 2, pairs) == LR_ERR_ARG);
    R(lr_setup_rkg_round3(s, nullptr, u, sk, e, 2, polys) == LR_ERR_ARG);
    R(lr_setup_rkg_round3_device(s, r2, u, sk, nullptr, 2, polys) == LR_ERR_ARG);
    R(lr_setup_rkg_key(s, nullptr, r3, evk) == LR_ERR_ARG);
    R(lr_setup_rkg_key(s, r2, nullptr, evk) == LR_ERR_ARG);
    R(lr_setup_rkg_key(s, r2, r3, nullptr) == LR_ERR_ARG);
    R(lr_setup_rkg_naive_round1(s, LR_SETUP_BFV, sk, nullptr, pk1, e, e, e, 2, pairs) == LR_ERR_ARG);
    R(lr_setup_rkg_naive_round1(s, LR_SETUP_BFV, sk, pk0, nullptr, e, e, e, 2, pairs) == LR_ERR_ARG);
    R(lr_setup_rkg_naive_round1_device(s, LR_SETUP_CKKS, sk, pk0, pk1, e, nullptr, e, 2, pairs) == LR_ERR_ARG);
    R(lr_setup_rkg_naive_round1_device(s, LR_SETUP_CKKS, sk, pk0, pk1, e, e, nullptr, 2, pairs) == LR_ERR_ARG);
    R(lr_setup_rkg_naive_round2(s, nullptr, sk, pk0, pk1, e, e, e, 2, pairs) == LR_ERR_ARG);
    R(lr_setup_rkg_naive_round2_device(s, r2, sk, pk0, pk1, e, e, nullptr, 2, pairs) == LR_ERR_ARG);
    R(lr_setup_rkg_naive_key(s, nullptr, evk) == LR_ERR_ARG);
    R(lr_setup_rkg_naive_key(s, r2, nullptr) == LR_ERR_ARG);
    R(lr_setup_rtg_share(s, nullptr, g, 2, crp, e, polys) == LR_ERR_ARG);
    R(lr_setup_rtg_share(s, sk1, nullptr, 2, crp, e, polys) == LR_ERR_ARG);
    R(lr_setup_rtg_share_device(s, sk1, g, 2, nullptr, e, polys) == LR_ERR_ARG);
    R(lr_setup_rtg_share_device(s, sk1, g, 2, crp, nullptr, polys) == LR_ERR_ARG);
    R(lr_setup_rtg_key(s, nullptr, crp, evk) == LR_ERR_ARG);
    R(lr_setup_rtg_key(s, r1, nullptr, evk) == LR_ERR_ARG);
    R(lr_setup_rtg_key(s, r1, crp, nullptr) == LR_ERR_ARG);
    R(lr_setup_aggregate(s, nullptr, 2, r1) == LR_ERR_ARG);
    R(lr_setup_aggregate(s, shares, 2, nullptr) == LR_ERR_ARG);
    {
        const lr_poly *holes[2] = {r1, nullptr};
        R(lr_setup_aggregate(s, holes, 2, r1) == LR_ERR_ARG);
    }
    // a poly of another context, an output that is an input or another output, an even Galois element, an unknown scheme
    R(lr_setup_ckg_share(s, foreign, crs, e, 2, ckg) == LR_ERR_ARG);
    R(lr_setup_ckg_share(s, sk, foreign1, e, 2, ckg) == LR_ERR_ARG);
    R(lr_setup_ckg_share(s, sk, crs, e, 2, foreign) == LR_ERR_ARG);
    R(lr_setup_ckg_share(s, sk, crs, e, 2, sk) == LR_ERR_ARG);
    R(lr_setup_rkg_round1(s, foreign, sk, crp, e, 2, polys) == LR_ERR_ARG);
    R(lr_setup_rkg_round1(s, u, sk, fshare, e, 2, polys) == LR_ERR_ARG);
    R(lr_setup_rkg_round1(s, u, sk, crp, e, 2, with_foreign) == LR_ERR_ARG);
    R(lr_setup_rkg_round1(s, u, sk, crp, e, 2, same) == LR_ERR_ARG);
    R(lr_setup_rkg_round1(s, inside, sk1, crp, e, 1, one) == LR_ERR_ARG);
    R(lr_setup_rkg_round1(s, u, sk, a1, e, 2, polys) == LR_ERR_ARG);                    // crp is a share
    R(lr_setup_rkg_round2(s, fshare, sk, crp, e, 2, pairs) == LR_ERR_ARG);
    R(lr_setup_rkg_round3(s, fpair, u, sk, e, 2, polys) == LR_ERR_ARG);
    R(lr_setup_rkg_round3(s, r2, sk1, inside, e, 1, one) == LR_ERR_ARG);
    R(lr_setup_rkg_key(s, r2, r3, fpair) == LR_ERR_ARG);
    R(lr_setup_rkg_key(s, head, r3, tail) == LR_ERR_ARG);                               // a partial overlap
    R(lr_setup_rkg_naive_key(s, head, tail) == LR_ERR_ARG);
    R(lr_setup_rkg_naive_round1(s, 2, sk, pk0, pk1, e, e, e, 2, pairs) == LR_ERR_ARG);
    R(lr_setup_rkg_naive_round1(s, LR_SETUP_BFV, sk, foreign1, pk1, e, e, e, 2, pairs) == LR_ERR_ARG);
    R(lr_setup_rkg_naive_round2(s, b0, sk, pk0, pk1, e, e, e, 2, pairs) == LR_ERR_ARG);  // round1 is a share
    R(lr_setup_rtg_share(s, sk1, even, 2, crp, e, polys) == LR_ERR_ARG);
    R(lr_setup_rtg_share_device(s, sk1, zero, 2, crp, e, polys) == LR_ERR_ARG);
    R(lr_setup_rtg_key(s, r1, crp, fpair) == LR_ERR_ARG);
    R(lr_setup_aggregate(s, overl, 1, tail) == LR_ERR_ARG);
    // counts, batches and limbs
    R(lr_setup_ckg_share(s, sk, crs, e, 0, ckg) == LR_ERR_SHAPE);
    R(lr_setup_ckg_share(s, sk3, crs, e, 3, sk3) == LR_ERR_SHAPE);                      // above max_batch
    R(lr_setup_ckg_share(s, sk3, crs, e, 2, ckg) == LR_ERR_SHAPE);                      // a key whose batch is neither 1 nor n
    R(lr_setup_ckg_share(s, sk, crs, e, 2, narrow) == LR_ERR_SHAPE);
    R(lr_setup_rkg_round1(s, u, sk, crp, e, -1, polys) == LR_ERR_SHAPE);
    R(lr_setup_rkg_round1(s, u, sk, crp, e, 3, three) == LR_ERR_SHAPE);
    R(lr_setup_rkg_round1(s, sk3, sk, crp, e, 2, polys) == LR_ERR_SHAPE);
    R(lr_setup_rkg_round1(s, u, narrow, crp, e, 2, polys) == LR_ERR_SHAPE);
    R(lr_setup_rkg_round1(s, u, sk, r2, e, 2, polys) == LR_ERR_SHAPE);                  // crp of batch 2 beta
    R(lr_setup_rkg_round1(s, u, sk, crp, e, 2, pairs) == LR_ERR_SHAPE);                 // shares of pairs where polys are due
    R(lr_setup_rkg_round1(s, u, sk, crp, e, 2, with_narrow) == LR_ERR_SHAPE);
    R(lr_setup_rkg_round2(s, r2, sk, crp, e, 2, pairs) == LR_ERR_SHAPE);
    R(lr_setup_rkg_round2(s, r1, sk, crp, e, 2, polys) == LR_ERR_SHAPE);
    R(lr_setup_rkg_round3(s, r1, u, sk, e, 2, polys) == LR_ERR_SHAPE);
    R(lr_setup_rkg_round3(s, npair, u, sk, e, 2, polys) == LR_ERR_SHAPE);
    R(lr_setup_rkg_key(s, r2, r3, r1) == LR_ERR_SHAPE);
    R(lr_setup_rkg_key(s, r2, r2, evk) == LR_ERR_SHAPE);
    R(lr_setup_rkg_key(s, odd, r3, evk) == LR_ERR_SHAPE);
    R(lr_setup_rkg_naive_round1(s, LR_SETUP_BFV, sk, sk, pk1, e, e, e, 2, pairs) == LR_ERR_SHAPE);   // the public key has batch 1
    R(lr_setup_rkg_naive_round2(s, r1, sk, pk0, pk1, e, e, e, 2, pairs) == LR_ERR_SHAPE);
    R(lr_setup_rkg_naive_round2(s, r2, sk, pk0, pk1, e, e, e, 0, pairs) == LR_ERR_SHAPE);
    R(lr_setup_rkg_naive_key(s, r2, r1) == LR_ERR_SHAPE);
    R(lr_setup_rtg_share(s, sk, g, 2, crp, e, polys) == LR_ERR_SHAPE);                  // one secret key
    R(lr_setup_rtg_share(s, sk1, g, 3, crp, e, three) == LR_ERR_SHAPE);
    R(lr_setup_rtg_key(s, r2, crp, evk) == LR_ERR_SHAPE);
    R(lr_setup_rtg_key(s, r1, crp, r3) == LR_ERR_SHAPE);
    R(lr_setup_aggregate(s, shares, 0, r1) == LR_ERR_SHAPE);
    R(lr_setup_aggregate(s, mixed, 2, r1) == LR_ERR_SHAPE);
    R(lr_setup_aggregate(s, shares, 2, odd) == LR_ERR_SHAPE);                           // neither 1, beta nor 2 beta
    {   // the two contexts on different streams: every entry point of a handle with a ctxP refuses
        hipStream_t st = nullptr;
        CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
        OK(lr_context_set_stream(r.q, st));
        R(lr_setup_ckg_share(s, sk, crs, e, 2, ckg) == LR_ERR_ARG);
        CHECK(std::string(lr_last_error_string()).find("different streams") != std::string::npos);
        R(lr_setup_rkg_round1_device(s, u, sk, crp, e, 2, polys) == LR_ERR_ARG);
        R(lr_setup_rkg_round2(s, r1, sk, crp, e, 2, pairs) == LR_ERR_ARG);
        R(lr_setup_rkg_round3(s, r2, u, sk, e, 2, polys) == LR_ERR_ARG);
        R(lr_setup_rkg_key(s, r2, r3, r2) == LR_ERR_ARG);
        R(lr_setup_rkg_naive_round1(s, LR_SETUP_CKKS, sk, pk0, pk1, e, e, e, 2, pairs) == LR_ERR_ARG);
        R(lr_setup_rkg_naive_round2_device(s, r2, sk, pk0, pk1, e, e, e, 2, pairs) == LR_ERR_ARG);
        R(lr_setup_rkg_naive_key(s, r2, evk) == LR_ERR_ARG);
        R(lr_setup_rtg_share(s, sk1, g, 2, crp, e, polys) == LR_ERR_ARG);
        R(lr_setup_rtg_key(s, r1, crp, evk) == LR_ERR_ARG);
        R(lr_setup_aggregate(s, ones, 2, pk0) == LR_ERR_ARG);
        OK(lr_setup_ckg_share(no_p, skq, crsq, e, 2, ckgq));                            // a handle without ctxP has one stream
        OK(lr_context_sync(r.q));
        OK(lr_context_set_stream(r.q, nullptr));
        CHECK(hipStreamDestroy(st) == hipSuccess);
    }
#undef R
    // only the two accepted calls launched anything: expansion, transform, and (call-by-call or not) what follows it is not counted here
    CHECK(lr::g_stub_launches.load() + lr::g_ckks_expand_launches.load() + lr::g_fold_launches.load() - before == 4);
    OK(lr_setup_rkg_round1(s, u, sk, crp, e, 2, polys));                               // the handle stays usable
    OK(lr_setup_rkg_key(s, r2, r3, r2));
    for (lr_poly *p : {sk, u, sk1, sk3, crs, crp, ckg, r1, r2, r3, evk, pk0, pk1, foreign, foreign1, fshare, fpair, narrow, nshare, npair, odd, a0, a1,
                       a2, b0, b1, skq, crsq, ckgq, inside, head, tail})
        lr_poly_free(p);
    OK(lr_setup_destroy(no_p));
    OK(lr_setup_destroy(s));
    OK(lr_setup_destroy(nullptr));
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
        calls += exercise(N, 3, 2, &call_by_call);        // ragged: the last digit owns one row
    }
    calls += exercise(1 << 4, 3, 2, nullptr);
    calls += exercise(1 << 4, 3, 1, &call_by_call);
    calls += exercise(1 << 4, 3, 2, nullptr, 70);         // 70 parties: passes of 32, 32 and 6
    calls += exercise(1 << 4, 3, 1, &call_by_call, 70);
    sequences();
    refused += refusals();
    {   // two handles on two threads, each with its own contexts: nothing is shared but the library's globals
        std::atomic<int> threaded{0};
        std::thread a([&] { threaded += exercise(1 << 12, 3, 2, nullptr); });
        std::thread b([&] { threaded += exercise(1 << 4, 3, 1, &call_by_call); });
        a.join();
        b.join();
        calls += threaded.load();
    }
    return driver_end(ALLOCATIONS | EVENTS | LOG, refused, "setup: calls %d, refusals %d", calls, refused);
}
