// The BFV rotation chains' host side under AddressSanitizer + UBSan and under ThreadSanitizer (tests/test_host_bfv_chain_sanitizers.py): the
// REAL host code -- lr_abi_*.cpp (the chains are in lr_abi_bfv_eval.cpp), lr_host.hpp, lr_precompute.cpp -- compiled with g++ against the
// host-only HIP stand-in and the recording launch stubs of tests/cpp/hipstub/.  lr_bfv_inner_sum and lr_bfv_rotate_chain over
//   * N = 2^12 and 2^14 (the fused route), 2^15, 2^10 and 2 (the composed route; N = 2: the row step alone), |Q| = 5 with |P| = 3 or 2;
//   * the default plan, lr_options::no_epilogue (composed at every degree) and no_pair;
//   * batches 1, 2 and 5; out of place, in place, into the other component's poly, polys with another stride than the pools';
//   * accumulate and replace chains of 0, 1, 2 and 3 steps, one key handle for several steps;
//   * each entry point as the first call on a fresh plan and then at a larger batch (its pools are allocated, then moved, by that call);
//   * the number of step launches of each route, and that the last step of a chain writes no next input;
//   * every refusal of the header: the code, and that nothing was launched;
//   * two plans on two threads.
// Exit code 0 = every check held; a sanitizer report aborts the run.  Nothing here computes: parity is the GPU suite's business.
#include <thread>
#include <vector>

#include "driver_check.hpp"

namespace lr {
extern std::atomic<unsigned long long> g_bfv_chain_step_launches, g_bfv_chain_step_last, g_bfv_chain_step_crossed;
}

static const int MAXB = 5;

struct Ring {
    int logn;
    int nP;
    bool lds;      // a row fits the LDS: the fused route unless the options say otherwise
};
static const Ring kRings[5] = {{12, 3, true}, {14, 2, true}, {15, 2, false}, {10, 3, false}, {1, 2, false}};

struct Plan {
    Ring r;
    bool fused = false, pairs = true;
    // the route of a chain (chain_route, lr_abi_bfv_eval.cpp): a replace chain of one ciphertext at N = 2^14 takes the separate launches
    bool step_pass(int batch, int accumulate) const { return fused && !(accumulate == 0 && batch == 1 && r.logn == 14 && pairs); }
    lr_context *q = nullptr, *p = nullptr;
    lr_ckks_plan *pl = nullptr;
    lr_poly *key = nullptr, *key2 = nullptr;
    std::vector<const lr_poly *> cols;      // log2(N) - 1 handles, two different ones in turn
};

static Plan make(const Ring &r, const lr_options &opt) {
    Plan P;
    P.r = r;
    P.fused = r.lds && !opt.no_epilogue;
    P.pairs = !opt.no_pair;
    OK(lr_context_create_ex((uint64_t)1 << r.logn, Q5, 5, 0, &opt, &P.q));
    OK(lr_context_create_ex((uint64_t)1 << r.logn, P3, r.nP, 0, &opt, &P.p));
    OK(lr_ckks_plan_create_ex(P.q, P.p, MAXB, &opt, &P.pl));
    const int beta = (5 + r.nP - 1) / r.nP;
    P.key = poly(P.q, 5 + r.nP, 2 * beta);
    P.key2 = poly(P.q, 5 + r.nP, 2 * beta);
    for (int i = 0; i + 1 < r.logn; ++i) P.cols.push_back(i & 1 ? P.key2 : P.key);
    return P;
}
static void drop(Plan &P) {
    OK(lr_ckks_plan_destroy(P.pl));
    OK(lr_poly_free(P.key));
    OK(lr_poly_free(P.key2));
    OK(lr_context_destroy(P.q));
    OK(lr_context_destroy(P.p));
}

static int inner(const Plan &P, const lr_poly *c0, const lr_poly *c1, lr_poly *o0, lr_poly *o1) {
    return lr_bfv_inner_sum(P.pl, c0, c1, (int)P.cols.size(), P.cols.empty() ? nullptr : P.cols.data(), P.key, o0, o1);
}
static int chain(const Plan &P, const lr_poly *c0, const lr_poly *c1, int n, int accumulate, lr_poly *o0, lr_poly *o1) {
    const uint64_t gens[3] = {5, 25, ((uint64_t)2 << P.r.logn) - 1};
    const lr_poly *keys[3] = {P.key, P.key, P.key2};
    return lr_bfv_rotate_chain(P.pl, c0, c1, n, gens, keys, accumulate, o0, o1);
}

// every shape of call at one batch; `counted`: the launch counters are this thread's alone
static void calls(const Plan &P, int batch, bool counted) {
    lr_context *q = P.q;
    lr_poly *a0 = poly(q, 5, batch), *a1 = poly(q, 5, batch), *o0 = poly(q, 5, batch), *o1 = poly(q, 5, batch);
    lr_poly *w0 = poly(q, 6, batch), *w1 = poly(q, 6, batch);                       // another poly stride than the pools'
    const unsigned long long steps0 = lr::g_bfv_chain_step_launches.load(), last0 = lr::g_bfv_chain_step_last.load();
    unsigned long long steps = 0, chains = 0;
    auto ran = [&](int n, int acc) {
        if (!P.step_pass(batch, acc)) return;
        steps += (unsigned long long)n;
        chains += n > 0;
    };
    const int n_sum = P.r.logn;                                                      // log2(N) - 1 column steps and the row step
    RUN(inner(P, a0, a1, o0, o1)); ran(n_sum, 1);
    RUN(inner(P, a0, a1, a0, a1)); ran(n_sum, 1);                                    // in place
    RUN(inner(P, a0, a1, a1, a0)); ran(n_sum, 1);                                    // into the other component's poly
    RUN(inner(P, a0, a1, o0, a0)); ran(n_sum, 1);
    RUN(inner(P, w0, a1, o0, w1)); ran(n_sum, 1);
    RUN(inner(P, a0, a0, o0, o1)); ran(n_sum, 1);                                    // the same component twice
    for (int acc = 0; acc < 2; ++acc)
        for (int n = 0; n <= 3; ++n) {
            RUN(chain(P, a0, a1, n, acc, o0, o1)); ran(n, acc);
            RUN(chain(P, a0, a1, n, acc, a0, a1)); ran(n, acc);
            RUN(chain(P, a0, a1, n, acc, a1, a0)); ran(n, acc);
            RUN(chain(P, w0, w1, n, acc, w0, o1)); ran(n, acc);
        }
    if (counted) {
        CHECK(lr::g_bfv_chain_step_launches.load() - steps0 == steps);
        CHECK(lr::g_bfv_chain_step_last.load() - last0 == chains);                     // one step per chain writes no next input: the last
    }
    for (lr_poly *x : {a0, a1, o0, o1, w0, w1}) OK(lr_poly_free(x));
}

static void refusals(const Plan &P) {
    lr_context *q = P.q;
    lr_ckks_plan *pl = P.pl;
    lr_poly *a0 = poly(q, 5, 2), *a1 = poly(q, 5, 2), *o0 = poly(q, 5, 2), *o1 = poly(q, 5, 2), *narrow = poly(q, 4, 2), *three = poly(q, 5, 3);
    lr_poly *big[4];
    for (lr_poly *&x : big) x = poly(q, 5, MAXB + 1);
    lr_context *other = nullptr;
    OK(lr_context_create(P.r.logn > 1 ? (uint64_t)1 << (P.r.logn - 1) : 4, Q5, 5, 0, &other));      // another degree
    lr_poly *foreign = poly(other, 5, 2);
    const uint64_t gens[2] = {5, 25}, even[2] = {5, 6};
    const lr_poly *keys[2] = {P.key, P.key2}, *holed[2] = {P.key, nullptr};
    const int nc = (int)P.cols.size();
    const lr_poly *const *cols = nc ? P.cols.data() : nullptr;

    REFUSED(lr_bfv_rotate_chain(nullptr, a0, a1, 2, gens, keys, 1, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_rotate_chain(pl, nullptr, a1, 2, gens, keys, 1, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_rotate_chain(pl, a0, a1, 2, gens, keys, 1, o0, nullptr), LR_ERR_ARG);
    REFUSED(lr_bfv_rotate_chain(pl, a0, a1, 2, nullptr, keys, 1, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_rotate_chain(pl, a0, a1, 2, gens, nullptr, 1, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_rotate_chain(pl, a0, a1, 2, gens, holed, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_rotate_chain(pl, a0, a1, -1, gens, keys, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_rotate_chain(pl, a0, a1, 2, even, keys, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_rotate_chain(pl, a0, a1, 2, gens, keys, 0, o0, o0), LR_ERR_ARG);
    REFUSED(lr_bfv_rotate_chain(pl, big[0], big[1], 2, gens, keys, 0, big[2], big[2]), LR_ERR_ARG);       // two reasons: the argument checks come first
    REFUSED(lr_bfv_rotate_chain(pl, big[0], big[1], 2, gens, keys, 0, big[2], big[3]), LR_ERR_SHAPE);
    REFUSED(lr_bfv_rotate_chain(pl, big[0], big[1], 0, nullptr, nullptr, 0, big[2], big[3]), LR_ERR_SHAPE);
    REFUSED(lr_bfv_rotate_chain(pl, a0, narrow, 2, gens, keys, 1, o0, o1), LR_ERR_SHAPE);
    REFUSED(lr_bfv_rotate_chain(pl, a0, a1, 2, gens, keys, 1, narrow, o1), LR_ERR_SHAPE);
    REFUSED(lr_bfv_rotate_chain(pl, a0, a1, 2, gens, keys, 1, o0, three), LR_ERR_SHAPE);
    REFUSED(lr_bfv_rotate_chain(pl, foreign, a1, 2, gens, keys, 1, o0, o1), LR_ERR_SHAPE);

    REFUSED(lr_bfv_inner_sum(nullptr, a0, a1, nc, cols, P.key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_inner_sum(pl, a0, nullptr, nc, cols, P.key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_inner_sum(pl, a0, a1, nc, cols, nullptr, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_inner_sum(pl, a0, a1, nc, cols, P.key, nullptr, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_inner_sum(pl, a0, a1, nc, cols, P.key, o1, o1), LR_ERR_ARG);
    {
        std::vector<const lr_poly *> more(P.cols);
        more.push_back(P.key2);
        REFUSED(lr_bfv_inner_sum(pl, a0, a1, nc + 1, more.data(), P.key, o0, o1), LR_ERR_ARG);            // one key too many
    }
    REFUSED(lr_bfv_inner_sum(pl, a0, a1, -1, cols, P.key, o0, o1), LR_ERR_ARG);
    if (nc > 0) {
        std::vector<const lr_poly *> hole(P.cols);
        hole.back() = nullptr;
        REFUSED(lr_bfv_inner_sum(pl, a0, a1, nc, nullptr, P.key, o0, o1), LR_ERR_ARG);
        REFUSED(lr_bfv_inner_sum(pl, a0, a1, nc, hole.data(), P.key, o0, o1), LR_ERR_ARG);
        REFUSED(lr_bfv_inner_sum(pl, a0, a1, nc - 1, cols, P.key, o0, o1), LR_ERR_ARG);
        REFUSED(lr_bfv_inner_sum(pl, big[0], big[1], nc - 1, cols, P.key, big[2], big[3]), LR_ERR_ARG);   // two reasons: the argument first
    }
    REFUSED(lr_bfv_inner_sum(pl, big[0], big[1], nc, cols, P.key, big[2], big[3]), LR_ERR_SHAPE);
    REFUSED(lr_bfv_inner_sum(pl, narrow, a1, nc, cols, P.key, o0, o1), LR_ERR_SHAPE);
    REFUSED(lr_bfv_inner_sum(pl, a0, a1, nc, cols, P.key, o0, foreign), LR_ERR_SHAPE);
    REFUSED(lr_bfv_inner_sum(pl, a0, three, nc, cols, P.key, o0, o1), LR_ERR_SHAPE);

    // the two contexts on different streams: a pipeline over both refuses
    hipStream_t s = nullptr;
    CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess);
    OK(lr_context_set_stream(q, s));
    REFUSED(lr_bfv_inner_sum(pl, a0, a1, nc, cols, P.key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_rotate_chain(pl, a0, a1, 2, gens, keys, 0, o0, o1), LR_ERR_ARG);
    OK(lr_context_set_stream(q, nullptr));
    CHECK(hipStreamDestroy(s) == hipSuccess);

    for (lr_poly *x : {a0, a1, o0, o1, narrow, three, foreign}) OK(lr_poly_free(x));
    for (lr_poly *x : big) OK(lr_poly_free(x));
    OK(lr_context_destroy(other));
}

// each entry point as the first call on a fresh plan, then at a larger batch: every pool it uses is allocated, and then moved, by this very call
static void cold(const Plan &P, const lr_options &opt) {
    for (int entry = 0; entry < 3; ++entry) {
        Plan F = P;
        OK(lr_ckks_plan_create_ex(P.q, P.p, MAXB, &opt, &F.pl));
        for (int batch : {2, MAXB}) {
            lr_poly *v[4];
            for (lr_poly *&x : v) x = poly(P.q, 5, batch);
            switch (entry) {
            case 0: RUN(inner(F, v[0], v[1], v[2], v[3])); break;
            case 1: RUN(chain(F, v[0], v[1], 3, 0, v[2], v[3])); break;
            default: RUN(chain(F, v[0], v[1], 0, 0, v[1], v[0])); break;
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
            for (int batch : {1, 2, MAXB}) calls(P, batch, true);
            refusals(P);
            cold(P, opt);
            if (g_fail.load() != fail_before) std::fprintf(stderr, "... at N = 2^%d, variant %d\n", r.logn, v);
            drop(P);
        }
    }
    CHECK(lr::g_bfv_chain_step_launches.load() > 0);
    // two plans on two threads, each over its own contexts
    {
        lr_options opt;
        OK(lr_options_init(&opt));
        Plan A = make(kRings[0], opt), B = make(kRings[3], opt);
        std::thread ta([&] { for (int batch : {1, MAXB}) calls(A, batch, false); });
        std::thread tb([&] { for (int batch : {1, MAXB}) calls(B, batch, false); });
        ta.join();
        tb.join();
        drop(A);
        drop(B);
    }
    CHECK(lr::g_bfv_chain_step_crossed.load() == 0);                       // no step pass ever got the other component's operand as an output
    return driver_end(ALLOCATIONS, g_refusals, "bfv_chain: calls %d, refusals %d, step launches %llu", g_calls.load(), g_refusals.load(),
                lr::g_bfv_chain_step_launches.load());
}
