// The CKKS rotation chain's host side under AddressSanitizer + UBSan and under ThreadSanitizer (tests/test_host_ckks_chain_sanitizers.py):
// the REAL host code -- lr_abi_*.cpp (the chain is in lr_abi_ckks_eval.cpp, the key switch in lr_abi_ckks.cpp), lr_host.hpp,
// lr_precompute.cpp -- compiled with g++ against the host-only HIP stand-in and the recording launch stubs of tests/cpp/hipstub/.
// lr_ckks_rotate_chain over
//   * N = 2^12, 2^14 and 2^15 (accumulating chains on the fused route) and 2^10 (no transform epilogue: composed), |Q| = 5 with |P| = 3 or 2;
//   * the default plan, lr_options::no_epilogue (composed at every degree) and no_pair;
//   * levels 0, 2 and the top; batches 1, 2 and max_batch;
//   * out of place, in place, into the other component's poly, polys with another stride than the pools' and than each other's;
//   * accumulate and replace chains of 0, 1, 2 and 3 steps, one key handle for several steps;
//   * the call as the first on a fresh plan and then at a larger batch (its pools are allocated, then moved, by that call);
//   * the number of step launches of each route: one per accumulating step on the fused route, none on the composed one or when replacing;
//   * every refusal of the header: the code, and that nothing was launched;
//   * two plans on two threads.
// Exit code 0 = every check held; a sanitizer report aborts the run.  Nothing here computes: parity is the GPU suite's business.
#include <thread>
#include <vector>

#include "driver_check.hpp"

namespace lr {
extern std::atomic<unsigned long long> g_ckks_chain_step_launches;
}

static const int MAXB = 5, NQ = 5;

struct Ring {
    int logn;
    int nP;
    bool epilogue;      // the forward transform has an epilogue: accumulating chains take the fused route unless the options say otherwise
};
static const Ring kRings[4] = {{12, 3, true}, {15, 2, true}, {14, 3, true}, {10, 3, false}};

struct Plan {
    Ring r;
    bool fused = false;
    lr_context *q = nullptr, *p = nullptr;
    lr_ckks_plan *pl = nullptr;
    lr_poly *key = nullptr, *key2 = nullptr;
};

static Plan make(const Ring &r, const lr_options &opt) {
    Plan P;
    P.r = r;
    P.fused = r.epilogue && !opt.no_epilogue;
    OK(lr_context_create_ex((uint64_t)1 << r.logn, Q5, NQ, 0, &opt, &P.q));
    OK(lr_context_create_ex((uint64_t)1 << r.logn, P3, r.nP, 0, &opt, &P.p));
    OK(lr_ckks_plan_create_ex(P.q, P.p, MAXB, &opt, &P.pl));
    const int beta = (NQ + r.nP - 1) / r.nP;
    P.key = poly(P.q, NQ + r.nP, 2 * beta);
    P.key2 = poly(P.q, NQ + r.nP, 2 * beta);
    return P;
}
static void drop(Plan &P) {
    OK(lr_ckks_plan_destroy(P.pl));
    OK(lr_poly_free(P.key));
    OK(lr_poly_free(P.key2));
    OK(lr_context_destroy(P.q));
    OK(lr_context_destroy(P.p));
}

static int chain(const Plan &P, int level, const lr_poly *c0, const lr_poly *c1, int n, int accumulate, lr_poly *o0, lr_poly *o1) {
    const uint64_t gens[3] = {5, 25, ((uint64_t)2 << P.r.logn) - 1};
    const lr_poly *keys[3] = {P.key, P.key, P.key2};
    return lr_ckks_rotate_chain(P.pl, level, c0, c1, n, gens, keys, accumulate, o0, o1);
}

// every shape of call at one level and batch; `counted`: the launch counters are this thread's alone
static void calls(const Plan &P, int level, int batch, bool counted) {
    lr_context *q = P.q;
    lr_poly *a0 = poly(q, NQ, batch), *a1 = poly(q, NQ, batch), *o0 = poly(q, NQ, batch), *o1 = poly(q, NQ, batch);
    lr_poly *w0 = poly(q, NQ + 1, batch), *w1 = poly(q, level + 1, batch);          // other strides than the pools', and than each other's
    const unsigned long long steps0 = lr::g_ckks_chain_step_launches.load();
    unsigned long long steps = 0;
    auto ran = [&](int n, int acc) {
        if (P.fused && acc) steps += (unsigned long long)n;      // (chain_route, lr_abi_ckks_eval.cpp: a replacing chain is composed everywhere)
    };
    for (int acc = 0; acc < 2; ++acc)
        for (int n = 0; n <= 3; ++n) {
            RUN(chain(P, level, a0, a1, n, acc, o0, o1)); ran(n, acc);
            RUN(chain(P, level, a0, a1, n, acc, a0, a1)); ran(n, acc);               // in place
            RUN(chain(P, level, a0, a1, n, acc, a1, a0)); ran(n, acc);               // into the other component's poly
            RUN(chain(P, level, a0, a1, n, acc, o0, a0)); ran(n, acc);
            RUN(chain(P, level, w0, w1, n, acc, w0, o1)); ran(n, acc);
            RUN(chain(P, level, a0, w1, n, acc, w1, w0)); ran(n, acc);
        }
    if (counted) {
        CHECK(lr::g_ckks_chain_step_launches.load() - steps0 == steps);               // one pass per step on the fused route, none otherwise
    }
    for (lr_poly *x : {a0, a1, o0, o1, w0, w1}) OK(lr_poly_free(x));
}

static void refusals(const Plan &P) {
    lr_context *q = P.q;
    lr_ckks_plan *pl = P.pl;
    const int top = NQ - 1;
    lr_poly *a0 = poly(q, NQ, 2), *a1 = poly(q, NQ, 2), *o0 = poly(q, NQ, 2), *o1 = poly(q, NQ, 2), *narrow = poly(q, NQ - 1, 2), *three = poly(q, NQ, 3);
    lr_poly *big[4];
    for (lr_poly *&x : big) x = poly(q, NQ, MAXB + 1);
    lr_context *other = nullptr;
    OK(lr_context_create((uint64_t)1 << (P.r.logn - 1), Q5, NQ, 0, &other));      // another degree
    lr_poly *foreign = poly(other, NQ, 2);
    const int beta = (NQ + P.r.nP - 1) / P.r.nP;
    lr_poly *few = poly(q, NQ + P.r.nP, 2 * beta - 1), *thin = poly(q, NQ + P.r.nP - 1, 2 * beta);      // key images that are too small
    const uint64_t gens[2] = {5, 25}, even[2] = {5, 6};
    const lr_poly *keys[2] = {P.key, P.key2}, *holed[2] = {P.key, nullptr}, *short_keys[2] = {P.key, few}, *thin_keys[2] = {thin, P.key};

    REFUSED(lr_ckks_rotate_chain(nullptr, top, a0, a1, 2, gens, keys, 1, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_rotate_chain(pl, top, nullptr, a1, 2, gens, keys, 1, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_rotate_chain(pl, top, a0, nullptr, 2, gens, keys, 1, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_rotate_chain(pl, top, a0, a1, 2, gens, keys, 1, nullptr, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_rotate_chain(pl, top, a0, a1, 2, gens, keys, 1, o0, nullptr), LR_ERR_ARG);
    REFUSED(lr_ckks_rotate_chain(pl, top, a0, a1, 2, nullptr, keys, 1, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_rotate_chain(pl, top, a0, a1, 2, gens, nullptr, 1, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_rotate_chain(pl, top, a0, a1, 2, gens, holed, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_rotate_chain(pl, top, a0, a1, -1, gens, keys, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_rotate_chain(pl, top, a0, a1, 2, even, keys, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_rotate_chain(pl, top, a0, a1, 2, gens, keys, 0, o0, o0), LR_ERR_ARG);
    REFUSED(lr_ckks_rotate_chain(pl, top, big[0], big[1], 2, gens, keys, 0, big[2], big[2]), LR_ERR_ARG);      // two reasons: the argument checks come first
    REFUSED(lr_ckks_rotate_chain(pl, top + 1, a0, a1, 2, even, keys, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_rotate_chain(pl, top + 1, a0, a1, 2, gens, keys, 0, o0, o1), LR_ERR_SHAPE);                 // level out of range
    REFUSED(lr_ckks_rotate_chain(pl, -1, a0, a1, 2, gens, keys, 0, o0, o1), LR_ERR_SHAPE);
    REFUSED(lr_ckks_rotate_chain(pl, top, big[0], big[1], 2, gens, keys, 0, big[2], big[3]), LR_ERR_SHAPE);     // a batch beyond max_batch
    REFUSED(lr_ckks_rotate_chain(pl, top, big[0], big[1], 0, nullptr, nullptr, 0, big[2], big[3]), LR_ERR_SHAPE);
    REFUSED(lr_ckks_rotate_chain(pl, top, a0, narrow, 2, gens, keys, 1, o0, o1), LR_ERR_SHAPE);                 // fewer limbs than level + 1
    REFUSED(lr_ckks_rotate_chain(pl, top, a0, a1, 2, gens, keys, 1, narrow, o1), LR_ERR_SHAPE);
    REFUSED(lr_ckks_rotate_chain(pl, top, a0, a1, 2, gens, keys, 1, o0, three), LR_ERR_SHAPE);                  // another batch
    REFUSED(lr_ckks_rotate_chain(pl, top, foreign, a1, 2, gens, keys, 1, o0, o1), LR_ERR_SHAPE);                // another degree
    REFUSED(lr_ckks_rotate_chain(pl, top, a0, a1, 2, gens, short_keys, 1, o0, o1), LR_ERR_SHAPE);               // a key image that is too small: the LAST step's,
    REFUSED(lr_ckks_rotate_chain(pl, top, a0, a1, 2, gens, thin_keys, 0, o0, o1), LR_ERR_SHAPE);                // and nothing was launched for the first
    RUN(lr_ckks_rotate_chain(pl, top - 1, a0, narrow, 2, gens, keys, 1, o0, narrow));                           // the narrow poly one level down: accepted

    // the two contexts on different streams: a pipeline over both refuses
    hipStream_t s = nullptr;
    CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess);
    OK(lr_context_set_stream(q, s));
    REFUSED(lr_ckks_rotate_chain(pl, top, a0, a1, 2, gens, keys, 0, o0, o1), LR_ERR_ARG);
    OK(lr_context_set_stream(q, nullptr));
    CHECK(hipStreamDestroy(s) == hipSuccess);

    for (lr_poly *x : {a0, a1, o0, o1, narrow, three, foreign, few, thin}) OK(lr_poly_free(x));
    for (lr_poly *x : big) OK(lr_poly_free(x));
    OK(lr_context_destroy(other));
}

// the call as the first on a fresh plan, then at a larger batch: every pool it uses is allocated, and then moved, by this very call
static void cold(const Plan &P, const lr_options &opt) {
    for (int entry = 0; entry < 3; ++entry) {
        Plan F = P;
        OK(lr_ckks_plan_create_ex(P.q, P.p, MAXB, &opt, &F.pl));
        for (int batch : {2, MAXB}) {
            lr_poly *v[4];
            for (lr_poly *&x : v) x = poly(P.q, NQ, batch);
            switch (entry) {
            case 0: RUN(chain(F, NQ - 1, v[0], v[1], 3, 1, v[2], v[3])); break;
            case 1: RUN(chain(F, 1, v[0], v[1], 1, 1, v[0], v[1])); break;                 // one accumulating step in place
            default: RUN(chain(F, NQ - 1, v[0], v[1], 0, 0, v[1], v[0])); break;
            }
            for (lr_poly *x : v) OK(lr_poly_free(x));
        }
        OK(lr_ckks_plan_destroy(F.pl));
    }
}

int main() {
    for (const Ring &r : kRings) {
        for (int v = 0; v < 3; ++v) {
            lr_options opt;
            OK(lr_options_init(&opt));
            if (v == 1) opt.no_epilogue = 1;
            if (v == 2) opt.no_pair = 1;
            Plan P = make(r, opt);
            const int fail_before = g_fail.load();
            for (int level : {0, 2, NQ - 1})
                for (int batch : {1, 2, MAXB}) calls(P, level, batch, true);
            refusals(P);
            cold(P, opt);
            if (g_fail.load() != fail_before) std::fprintf(stderr, "... at N = 2^%d, variant %d\n", r.logn, v);
            drop(P);
        }
    }
    CHECK(lr::g_ckks_chain_step_launches.load() > 0);
    // two plans on two threads, each over its own contexts
    {
        lr_options opt;
        OK(lr_options_init(&opt));
        Plan A = make(kRings[0], opt), B = make(kRings[3], opt);
        std::thread ta([&] { for (int batch : {1, MAXB}) calls(A, NQ - 1, batch, false); });
        std::thread tb([&] { for (int batch : {1, MAXB}) calls(B, 2, batch, false); });
        ta.join();
        tb.join();
        drop(A);
        drop(B);
    }
    return driver_end(ALLOCATIONS, g_refusals, "ckks_chain: calls %d, refusals %d, step launches %llu", g_calls.load(), g_refusals.load(),
                lr::g_ckks_chain_step_launches.load());
}
