// lr_bfv_relinearize_deg's host side under AddressSanitizer + UBSan and under ThreadSanitizer (tests/test_host_bfv_relin_deg_sanitizers.py):
// the REAL host code -- lr_abi_*.cpp (the call is in lr_abi_bfv_eval.cpp), lr_host.hpp, lr_precompute.cpp -- compiled with g++ against the
// host-only HIP stand-in and the recording launch stubs of tests/cpp/hipstub/.  Over
//   * N = 2^12, 2^15 and 8, |Q| = 5 with |P| = 3 or 2;
//   * the default plan (merged route), lr_options::no_epilogue (composed route) and no_pair;
//   * degrees 1 .. 5 at batches 1, 2 and max_batch, with max_batch 4 and 3: G = min(degree - 1, max(1, max_batch / batch)) takes 1, the
//     full degree - 1 and values between, with a partial last pass (degree 4 at G = 2, degree 5 at G = 3);
//   * out of place, in place, one output in place, polys with another stride than the pools';
//   * each degree as the first call on a fresh plan, then at a larger batch (its pools are allocated, then moved, by that call);
//   * the launch counts of each route: passes and terms of the fold, and the whole call against lr_bfv_relinearize's key switch on the same plan --
//     composed: (degree - 1) x (key switch + the Adds); merged: per pass the gather (G > 1), the key switch of G x batch members with
//     G - 1 further inner products, and one fold;
//   * every refusal of the header: the code, and that nothing was launched;
//   * two plans on two threads.
// Exit code 0 = every check held; a sanitizer report aborts the run.  Nothing here computes: parity is the GPU suite's business.
#include <algorithm>
#include <thread>
#include <vector>

#include "driver_check.hpp"

namespace lr {
extern std::atomic<unsigned long long> g_bfv_relin_fold_launches, g_bfv_relin_fold_terms, g_bfv_relin_fold_crossed;
}


struct Ring {
    int logn;
    int nP;
};
static const Ring kRings[3] = {{12, 3}, {15, 2}, {3, 3}};

struct Plan {
    Ring r;
    int maxb = 0;
    bool merged = false, pairs = true;
    lr_context *q = nullptr, *p = nullptr;
    lr_ckks_plan *pl = nullptr;
    lr_poly *key[4] = {nullptr, nullptr, nullptr, nullptr};      // the keys from s^2 .. s^5
};

static Plan make(const Ring &r, const lr_options &opt, int maxb) {
    Plan P;
    P.r = r;
    P.maxb = maxb;
    P.merged = !opt.no_epilogue;
    P.pairs = !opt.no_pair;
    OK(lr_context_create_ex((uint64_t)1 << r.logn, Q5, 5, 0, &opt, &P.q));
    OK(lr_context_create_ex((uint64_t)1 << r.logn, P3, r.nP, 0, &opt, &P.p));
    OK(lr_ckks_plan_create_ex(P.q, P.p, maxb, &opt, &P.pl));
    const int beta = (5 + r.nP - 1) / r.nP;
    for (lr_poly *&k : P.key) k = poly(P.q, 5 + r.nP, 2 * beta);
    return P;
}
static void drop(Plan &P) {
    OK(lr_ckks_plan_destroy(P.pl));
    for (lr_poly *k : P.key) OK(lr_poly_free(k));
    OK(lr_context_destroy(P.q));
    OK(lr_context_destroy(P.p));
}

static int relin(const Plan &P, const std::vector<lr_poly *> &ct, int degree, lr_poly *o0, lr_poly *o1) {
    const lr_poly *cts[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k <= degree; ++k) cts[k] = ct[(size_t)k];
    return lr_bfv_relinearize_deg(P.pl, cts, degree, degree >= 2 ? P.key : nullptr, o0, o1);
}

// the launches of one key switch of `members` polys into the plan's own accumulators (back to back: the tail takes both at once), read
// off lr_bfv_relinearize on this plan -- the key switch and its Adds -- warm: the second of two calls
static unsigned long long key_switch_launches(const Plan &P, int members) {
    lr_poly *c0 = poly(P.q, 5, members), *c1 = poly(P.q, 5, members), *c2 = poly(P.q, 5, members), *o0 = poly(P.q, 5, members), *o1 = poly(P.q, 5, members);
    OK(lr_bfv_relinearize(P.pl, c0, c1, c2, P.key[0], o0, o1));
    const unsigned long long before = lr::g_stub_launches.load();
    OK(lr_bfv_relinearize(P.pl, c0, c1, c2, P.key[0], o0, o1));
    const unsigned long long n = lr::g_stub_launches.load() - before - ((members == 1 && P.pairs) ? 1 : 2);
    for (lr_poly *y : {c0, c1, c2, o0, o1}) OK(lr_poly_free(y));
    return n;
}

// every shape of call at one batch; `counted`: the launch counters are this thread's alone
static void calls(const Plan &P, int batch, bool counted) {
    lr_context *q = P.q;
    std::vector<lr_poly *> ct, wide;
    for (int k = 0; k < 6; ++k) ct.push_back(poly(q, 5, batch));
    for (int k = 0; k < 6; ++k) wide.push_back(poly(q, 6, batch));                  // another poly stride than the pools'
    lr_poly *o0 = poly(q, 5, batch), *o1 = poly(q, 5, batch), *w0 = poly(q, 6, batch);
    // one inner product is one launch (the pair form) where pairs are on: batch x 5 rows stay below pair_max_workgroups here
    const unsigned long long ip = P.pairs ? 1 : 2, adds = (batch == 1 && P.pairs) ? 1 : 2;
    std::vector<unsigned long long> ks((size_t)P.maxb + 1, 0);
    if (counted)
        for (int m = batch; m <= P.maxb; m += batch) ks[(size_t)m] = key_switch_launches(P, m);
    for (int degree = 1; degree <= 5; ++degree) {
        unsigned long long want = 0, passes = 0, terms = 0;
        if (degree == 1) {
            want = 2;                                                                // two copies
        } else if (!P.merged) {
            want = (unsigned long long)(degree - 1) * (ks[(size_t)batch] + adds);
        } else {
            const int G = std::min(degree - 1, std::max(1, P.maxb / batch));
            for (int top = degree; top > 1;) {
                const int g = std::min(G, top - 1);
                want += (g > 1) + ks[(size_t)(g * batch)] + (unsigned long long)(g - 1) * ip + 1;
                ++passes;
                terms += (unsigned long long)g;
                top -= g;
            }
        }
        const unsigned long long l0 = lr::g_stub_launches.load(), f0 = lr::g_bfv_relin_fold_launches.load(), t0 = lr::g_bfv_relin_fold_terms.load();
        RUN(relin(P, ct, degree, o0, o1));
        if (counted) {
            CHECK(lr::g_stub_launches.load() - l0 == want);
            CHECK(lr::g_bfv_relin_fold_launches.load() - f0 == passes);
            CHECK(lr::g_bfv_relin_fold_terms.load() - t0 == terms);
        }
        RUN(relin(P, ct, degree, ct[0], ct[1]));                                     // in place
        RUN(relin(P, ct, degree, ct[0], o1));                                        // one output in place
        RUN(relin(P, ct, degree, o0, ct[1]));
        RUN(relin(P, wide, degree, o0, w0));                                         // other strides, in and out
        RUN(relin(P, wide, degree, wide[0], wide[1]));
        if (degree >= 3) {
            std::vector<lr_poly *> twice(ct);
            twice[2] = twice[3];                                                     // one input poly at two degrees
            RUN(relin(P, twice, degree, o0, o1));
        }
    }
    for (lr_poly *x : ct) OK(lr_poly_free(x));
    for (lr_poly *x : wide) OK(lr_poly_free(x));
    for (lr_poly *x : {o0, o1, w0}) OK(lr_poly_free(x));
}

static void refusals(const Plan &P) {
    lr_context *q = P.q;
    lr_ckks_plan *pl = P.pl;
    const int B = 1, beta = (5 + P.r.nP - 1) / P.r.nP;
    lr_poly *c[6], *big[6];
    for (lr_poly *&x : c) x = poly(q, 5, B);
    for (lr_poly *&x : big) x = poly(q, 5, P.maxb + 1);
    lr_poly *o0 = poly(q, 5, B), *o1 = poly(q, 5, B), *narrow = poly(q, 4, B), *more = poly(q, 5, B + 1);
    lr_poly *bigo0 = poly(q, 5, P.maxb + 1), *bigo1 = poly(q, 5, P.maxb + 1);
    lr_poly *thin_key = poly(q, 5 + P.r.nP - 1, 2 * beta), *short_key = poly(q, 5 + P.r.nP, 2 * beta - 1);
    lr_context *other = nullptr;
    OK(lr_context_create((uint64_t)1 << (P.r.logn - 1), Q5, 5, 0, &other));          // another degree
    lr_poly *foreign = poly(other, 5, B);
    const lr_poly *cts[6] = {c[0], c[1], c[2], c[3], c[4], c[5]}, *bigs[6] = {big[0], big[1], big[2], big[3], big[4], big[5]};
    const lr_poly *const *keys = P.key;
    auto with = [&](int k, const lr_poly *p) {
        std::vector<const lr_poly *> v(cts, cts + 6);
        v[(size_t)k] = p;
        return v;
    };

    REFUSED(lr_bfv_relinearize_deg(nullptr, cts, 3, keys, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_relinearize_deg(pl, nullptr, 3, keys, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_relinearize_deg(pl, cts, 3, keys, nullptr, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_relinearize_deg(pl, cts, 3, keys, o0, nullptr), LR_ERR_ARG);
    for (int k = 0; k <= 3; ++k) REFUSED(lr_bfv_relinearize_deg(pl, with(k, nullptr).data(), 3, keys, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_relinearize_deg(pl, cts, 2, nullptr, o0, o1), LR_ERR_ARG);
    {
        const lr_poly *holed[4] = {P.key[0], nullptr, P.key[2], P.key[3]};
        REFUSED(lr_bfv_relinearize_deg(pl, cts, 3, holed, o0, o1), LR_ERR_ARG);
        RUN(lr_bfv_relinearize_deg(pl, cts, 2, holed, o0, o1));                      // (the hole is beyond what degree 2 reads)
    }
    REFUSED(lr_bfv_relinearize_deg(pl, cts, 0, keys, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_relinearize_deg(pl, cts, 6, keys, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_relinearize_deg(pl, cts, -1, keys, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_relinearize_deg(pl, cts, 3, keys, o0, o0), LR_ERR_ARG);
    REFUSED(lr_bfv_relinearize_deg(pl, cts, 1, nullptr, o0, o0), LR_ERR_ARG);
    REFUSED(lr_bfv_relinearize_deg(pl, cts, 3, keys, c[2], o1), LR_ERR_ARG);         // an output that is ct[k], k >= 2
    REFUSED(lr_bfv_relinearize_deg(pl, cts, 3, keys, o0, c[3]), LR_ERR_ARG);
    RUN(lr_bfv_relinearize_deg(pl, cts, 2, keys, c[3], o1));                         // (ct[3] is no input at degree 2)
    REFUSED(lr_bfv_relinearize_deg(pl, cts, 3, keys, c[1], o1), LR_ERR_ARG);         // out0 being ct[1]
    REFUSED(lr_bfv_relinearize_deg(pl, cts, 3, keys, o0, c[0]), LR_ERR_ARG);         // out1 being ct[0]
    REFUSED(lr_bfv_relinearize_deg(pl, cts, 1, nullptr, c[1], c[0]), LR_ERR_ARG);
    REFUSED(lr_bfv_relinearize_deg(pl, bigs, 3, keys, bigo0, bigo0), LR_ERR_ARG);    // two reasons: the argument checks come first
    REFUSED(lr_bfv_relinearize_deg(pl, bigs, 3, keys, bigo0, bigo1), LR_ERR_SHAPE);
    REFUSED(lr_bfv_relinearize_deg(pl, bigs, 1, nullptr, bigo0, bigo1), LR_ERR_SHAPE);
    for (int k = 0; k <= 3; ++k) {
        REFUSED(lr_bfv_relinearize_deg(pl, with(k, narrow).data(), 3, keys, o0, o1), LR_ERR_SHAPE);
        REFUSED(lr_bfv_relinearize_deg(pl, with(k, foreign).data(), 3, keys, o0, o1), LR_ERR_SHAPE);
    }
    REFUSED(lr_bfv_relinearize_deg(pl, with(2, more).data(), 3, keys, o0, o1), LR_ERR_SHAPE);
    REFUSED(lr_bfv_relinearize_deg(pl, cts, 3, keys, narrow, o1), LR_ERR_SHAPE);
    REFUSED(lr_bfv_relinearize_deg(pl, cts, 3, keys, o0, more), LR_ERR_SHAPE);
    REFUSED(lr_bfv_relinearize_deg(pl, cts, 3, keys, foreign, o1), LR_ERR_SHAPE);
    {
        const lr_poly *thin[4] = {P.key[0], thin_key, P.key[2], P.key[3]}, *shrt[4] = {short_key, P.key[1], P.key[2], P.key[3]};
        REFUSED(lr_bfv_relinearize_deg(pl, cts, 3, thin, o0, o1), LR_ERR_SHAPE);     // a key image with fewer than |Q| + |P| limbs
        REFUSED(lr_bfv_relinearize_deg(pl, cts, 3, shrt, o0, o1), LR_ERR_SHAPE);     // ... with a batch below 2 beta
        REFUSED(lr_bfv_relinearize_deg(pl, cts, 3, thin, o0, o0), LR_ERR_ARG);       // two reasons: the argument first
    }

    // the two contexts on different streams: a pipeline over both refuses
    hipStream_t s = nullptr;
    CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess);
    OK(lr_context_set_stream(q, s));
    REFUSED(lr_bfv_relinearize_deg(pl, cts, 3, keys, o0, o1), LR_ERR_ARG);
    OK(lr_context_set_stream(q, nullptr));
    CHECK(hipStreamDestroy(s) == hipSuccess);

    for (lr_poly *x : c) OK(lr_poly_free(x));
    for (lr_poly *x : big) OK(lr_poly_free(x));
    for (lr_poly *x : {o0, o1, narrow, more, bigo0, bigo1, thin_key, short_key, foreign}) OK(lr_poly_free(x));
    OK(lr_context_destroy(other));
}

// each degree as the first call on a fresh plan, then at a larger batch: every pool it uses is allocated, and then moved, by this very call
static void cold(const Plan &P, const lr_options &opt) {
    for (int degree = 1; degree <= 5; ++degree) {
        Plan F = P;
        OK(lr_ckks_plan_create_ex(P.q, P.p, P.maxb, &opt, &F.pl));
        for (int batch : {1, P.maxb}) {
            std::vector<lr_poly *> ct;
            for (int k = 0; k < 6; ++k) ct.push_back(poly(P.q, 5, batch));
            lr_poly *o0 = poly(P.q, 5, batch), *o1 = poly(P.q, 5, batch);
            RUN(relin(F, ct, degree, o0, o1));
            for (lr_poly *x : ct) OK(lr_poly_free(x));
            for (lr_poly *x : {o0, o1}) OK(lr_poly_free(x));
        }
        OK(lr_ckks_plan_destroy(F.pl));
    }
}

int main() {
    for (const Ring &r : kRings) {
        for (int v = 0; v < 3; ++v) {
            for (int maxb : {4, 3}) {
                lr_options opt;
                OK(lr_options_init(&opt));
                if (v == 1) opt.no_epilogue = 1;
                if (v == 2) opt.no_pair = 1;
                Plan P = make(r, opt, maxb);
                const int fail_before = g_fail.load();
                for (int batch : {1, 2, maxb}) calls(P, batch, true);
                refusals(P);
                cold(P, opt);
                if (g_fail.load() != fail_before) std::fprintf(stderr, "... at N = 2^%d, variant %d, max_batch %d\n", r.logn, v, maxb);
                drop(P);
            }
        }
    }
    CHECK(lr::g_bfv_relin_fold_launches.load() > 0);
    // two plans on two threads, each over its own contexts
    {
        lr_options opt;
        OK(lr_options_init(&opt));
        Plan A = make(kRings[0], opt, 4), B = make(kRings[2], opt, 3);
        std::thread ta([&] { for (int batch : {1, 4}) calls(A, batch, false); });
        std::thread tb([&] { for (int batch : {1, 3}) calls(B, batch, false); });
        ta.join();
        tb.join();
        drop(A);
        drop(B);
    }
    CHECK(lr::g_bfv_relin_fold_crossed.load() == 0);                       // no fold ever got a term or the other component as an output
    return driver_end(ALLOCATIONS, g_refusals, "bfv_relin_deg: calls %d, refusals %d, fold launches %llu", g_calls.load(), g_refusals.load(),
                lr::g_bfv_relin_fold_launches.load());
}
