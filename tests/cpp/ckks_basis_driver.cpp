// The CKKS power basis' host side under AddressSanitizer + UBSan and under ThreadSanitizer (tests/test_host_ckks_basis_sanitizers.py):
// the REAL host code -- lr_abi_*.cpp (the basis, MulRelin and Rescale are in lr_abi_ckks_eval.cpp and lr_abi_ckks_scalar.cpp, the key switch
// in lr_abi_ckks.cpp, the division in lr_abi_ring.cpp), lr_host.hpp, lr_precompute.cpp -- compiled with g++ against the host-only HIP
// stand-in and the recording launch stubs of tests/cpp/hipstub/.  lr_ckks_power_basis_schedule and lr_ckks_power_basis over
//   * N = 2^12, 2^15 and 2^14 (the merged route) and 2^10 (no transform epilogue: composed), |Q| = 5 with |P| = 3 or 2;
//   * the default plan and lr_options::no_epilogue (composed at every degree);
//   * Chebyshev and monomial schedules with a layer of four products, C[1] at the top level and below it, scales that make products
//     rescale not at all, once and twice; outputs of exactly level_after + 1 limbs and of |Q| limbs;
//   * max_batch = batch, 2 * batch and 8 * batch: one product per chunk, two, the whole layer; a call whose widest chunk is a pair at a batch of 8,
//     which runs product by product;
//   * the call as the first on a fresh plan (its pools and table slots are allocated, then grown, by that call); a call takes at most
//     three table slots here, the eight slots wrap across the calls on one plan (the copies of this stand-in complete at once: what a
//     wrapped slot guards against is the GPU suite's to see);
//   * the launch counts of each route: per chunk of two products or more one tail launch and, on a schedule without divisions and tails,
//     exactly the launches of one lr_ckks_mulrelin over the chunk's members besides it; a chunk of one product as the composed route
//     runs it; on the composed route one combine launch per Chebyshev product and no tail launch;
//   * every refusal of the two headers: the code, and that nothing was launched;
//   * two plans on two threads.
// Exit code 0 = every check held; a sanitizer report aborts the run.  Nothing here computes: parity is the GPU suite's business.
#include <map>
#include <thread>
#include <tuple>
#include <vector>

#include "driver_check.hpp"

namespace lr {
extern std::atomic<unsigned long long> g_ckks_basis_tail_launches, g_ckks_basis_tail_products, g_combine_launches;
}

static const int NQ = 5, BATCH = 2;

struct Ring {
    int logn;
    int nP;
    bool epilogue;      // the forward transform has an epilogue: the merged route unless the options say otherwise
};
static const Ring kRings[4] = {{12, 3, true}, {15, 2, true}, {14, 3, true}, {10, 3, false}};

struct Plan {
    Ring r;
    bool merged = false;
    int max_batch = 0;
    lr_context *q = nullptr, *p = nullptr;
    lr_ckks_plan *pl = nullptr;
    lr_poly *key = nullptr;
};

static Plan make(const Ring &r, const lr_options &opt, int max_batch) {
    Plan P;
    P.r = r;
    P.merged = r.epilogue && !opt.no_epilogue;
    P.max_batch = max_batch;
    OK(lr_context_create_ex((uint64_t)1 << r.logn, Q5, NQ, 0, &opt, &P.q));
    OK(lr_context_create_ex((uint64_t)1 << r.logn, P3, r.nP, 0, &opt, &P.p));
    OK(lr_ckks_plan_create_ex(P.q, P.p, max_batch, &opt, &P.pl));
    P.key = poly(P.q, NQ + r.nP, 2 * ((NQ + r.nP - 1) / r.nP));
    return P;
}
static void drop(Plan &P) {
    OK(lr_ckks_plan_destroy(P.pl));
    OK(lr_poly_free(P.key));
    OK(lr_context_destroy(P.q));
    OK(lr_context_destroy(P.p));
}

struct Sched {
    int c1_level = 0;
    std::vector<lr_ckks_basis_product> p;
    std::vector<uint64_t> mult, add;      // rows of NQ words
    int n() const { return (int)p.size(); }
};

// the capacity protocol: ask with no room, then with exactly the room
static Sched schedule(int chebyshev, int c1_level, double c1_scale, const std::vector<uint32_t> &targets) {
    Sched S;
    S.c1_level = c1_level;
    int n = -1;
    const int rc = lr_ckks_power_basis_schedule(Q5, NQ, 1099511627776.0, chebyshev, c1_level, c1_scale, (int)targets.size(), targets.data(), 0, &n, nullptr,
                                                nullptr, nullptr);
    CHECK(n >= 0 && rc == (n == 0 ? LR_OK : LR_ERR_ARG));
    S.p.resize((size_t)n);
    S.mult.assign((size_t)n * NQ + 1, 0);
    S.add.assign((size_t)n * NQ + 1, 0);
    OK(lr_ckks_power_basis_schedule(Q5, NQ, 1099511627776.0, chebyshev, c1_level, c1_scale, (int)targets.size(), targets.data(), n, &n, S.p.data(),
                                    S.mult.data(), S.add.data()));
    CHECK(n == S.n());
    return S;
}

// products at level 0 without divisions and tails, written by hand: C[2] = C[1]^2, then C[3] = C[2] C[1] and C[4] = C[2]^2 in one layer
static Sched flat_schedule() {
    Sched S;
    S.c1_level = 0;
    const uint32_t abl[3][4] = {{2, 1, 1, 1}, {3, 2, 1, 2}, {4, 2, 2, 2}};
    for (const auto &r : abl) {
        lr_ckks_basis_product p{};
        p.n = r[0]; p.a = r[1]; p.b = r[2]; p.layer = (int32_t)r[3];
        S.p.push_back(p);
    }
    S.mult.assign(3 * NQ, 0);
    S.add.assign(3 * NQ, 0);
    return S;
}

// the chunks of the merged route: per group (layer, mul_level, n_rescales) its products, in the schedule's order, in pieces of per_chunk
static std::vector<std::vector<int>> chunks_of(const Sched &S, int per_chunk) {
    std::map<std::tuple<int, int, int>, std::vector<int>> groups;
    for (int k = 0; k < S.n(); ++k) groups[std::make_tuple(S.p[k].layer, -S.p[k].mul_level, S.p[k].n_rescales)].push_back(k);
    std::vector<std::vector<int>> out;
    for (const auto &g : groups)
        for (size_t k0 = 0; k0 < g.second.size(); k0 += (size_t)per_chunk)
            out.emplace_back(g.second.begin() + (long)k0, g.second.begin() + (long)std::min(g.second.size(), k0 + (size_t)per_chunk));
    return out;
}

struct Outs {
    std::vector<lr_poly *> c0, c1;
    void free_all() {
        for (lr_poly *x : c0) OK(lr_poly_free(x));
        for (lr_poly *x : c1) OK(lr_poly_free(x));
    }
};
static Outs outputs(const Plan &P, const Sched &S, int batch, bool exact) {
    Outs o;
    for (const auto &p : S.p) {
        o.c0.push_back(poly(P.q, exact ? p.level_after + 1 : NQ, batch));
        o.c1.push_back(poly(P.q, exact ? p.level_after + 1 : NQ, batch));
    }
    return o;
}

static int basis(const Plan &P, const Sched &S, const lr_poly *c0, const lr_poly *c1, const Outs &o) {
    return lr_ckks_power_basis(P.pl, S.n(), S.p.data(), S.mult.data(), S.add.data(), NQ, S.c1_level, c0, c1, P.key, o.c0.data(), o.c1.data());
}

// one schedule on one plan, outputs of both sizes; `counted`: the launch counters are this thread's alone
static void run(const Plan &P, const Sched &S, int batch, bool counted) {
    lr_poly *c0 = poly(P.q, NQ, batch), *c1 = poly(P.q, S.c1_level + 1, batch);      // (two strides)
    for (bool exact : {true, false}) {
        Outs o = outputs(P, S, batch, exact);
        const unsigned long long t0 = lr::g_ckks_basis_tail_launches.load(), p0 = lr::g_ckks_basis_tail_products.load(), k0 = lr::g_combine_launches.load();
        RUN(basis(P, S, c0, c1, o));
        if (counted) {
            // merged: one tail launch per chunk of two products or more; a chunk of one is the product as the composed route runs it
            unsigned long long launches = 0, products = 0, combines = 0;
            const auto chunks = chunks_of(S, std::max(1, P.max_batch / batch));
            size_t widest = 1;
            for (const auto &chunk : chunks) widest = std::max(widest, chunk.size());
            // (basis_route, lr_abi_ckks_eval.cpp: a call whose widest chunk is a pair, at a batch of 8 or more up to N = 2^15, merges nothing)
            const bool merges = P.merged && !(widest == 2 && batch >= 8 && P.r.logn <= 15);
            for (const auto &chunk : chunks) {
                if (merges && chunk.size() > 1) {
                    launches += 1;
                    products += chunk.size();
                } else {
                    for (int k : chunk) combines += S.p[k].tail != 0;
                }
            }
            CHECK(lr::g_ckks_basis_tail_launches.load() - t0 == launches);
            CHECK(lr::g_ckks_basis_tail_products.load() - p0 == products);
            CHECK(lr::g_combine_launches.load() - k0 == combines);
        }
        o.free_all();
    }
    OK(lr_poly_free(c0));
    OK(lr_poly_free(c1));
}

static std::vector<Sched> schedules() {
    const std::vector<uint32_t> wide = {2, 3, 4, 5, 6, 7, 8, 16};
    std::vector<Sched> v;
    for (int chebyshev = 0; chebyshev < 2; ++chebyshev) {
        v.push_back(schedule(chebyshev, NQ - 1, 281474976710656.0, wide));            // 2^48: C[2] is divided once, by the 55-bit limb
        v.push_back(schedule(chebyshev, NQ - 1, 295147905179352825856.0, {2, 3, 4})); // 2^68: C[2] is divided twice
        v.push_back(schedule(chebyshev, NQ - 1, 1099511627776.0, {2, 4}));            // 2^40 under the 55-bit limb: no division
        v.push_back(schedule(chebyshev, 2, 1099511627776.0, wide));                   // C[1] below the top: down to level 0 and stalled there
    }
    CHECK(v[1].p[0].n_rescales == 2 && v[2].p[0].n_rescales == 0 && v[0].p[0].n_rescales == 1);
    v.push_back(flat_schedule());
    v.push_back(schedule(1, NQ - 1, 1.0, {1}));                                       // nothing to do
    return v;
}

// a schedule without divisions and tails: besides the tail launch a chunk launches exactly what one MulRelin over its members does
static void tensor_count(const Plan &P) {
    if (!P.merged) return;
    const Sched S = flat_schedule();
    const int per_chunk = std::max(1, P.max_batch / BATCH);
    unsigned long long expect = 0;
    for (const auto &chunk : chunks_of(S, per_chunk)) {
        const int m = (int)chunk.size() * BATCH;
        lr_poly *x[6];
        for (lr_poly *&y : x) y = poly(P.q, 1, m);
        const unsigned long long before = lr::g_stub_launches.load();
        RUN(lr_ckks_mulrelin(P.pl, 0, x[0], x[1], x[2], x[3], P.key, x[4], x[5]));
        expect += lr::g_stub_launches.load() - before + (chunk.size() > 1 ? 1 : 0);
        for (lr_poly *y : x) OK(lr_poly_free(y));
    }
    lr_poly *c0 = poly(P.q, 1, BATCH), *c1 = poly(P.q, 1, BATCH);
    Outs o = outputs(P, S, BATCH, true);
    const unsigned long long before = lr::g_stub_launches.load();
    RUN(basis(P, S, c0, c1, o));
    CHECK(lr::g_stub_launches.load() - before == expect);
    o.free_all();
    OK(lr_poly_free(c0));
    OK(lr_poly_free(c1));
}

static void refusals(const Plan &P) {
    lr_context *q = P.q;
    lr_ckks_plan *pl = P.pl;
    const int top = NQ - 1;
    const Sched S = schedule(1, top, 281474976710656.0, {2, 3, 4});
    lr_poly *c0 = poly(q, NQ, BATCH), *c1 = poly(q, NQ, BATCH), *narrow = poly(q, 1, BATCH), *three = poly(q, NQ, 3);
    lr_poly *big0 = poly(q, NQ, P.max_batch + 1), *big1 = poly(q, NQ, P.max_batch + 1);
    lr_context *other = nullptr;
    OK(lr_context_create((uint64_t)1 << (P.r.logn - 1), Q5, NQ, 0, &other));      // another degree
    lr_poly *foreign = poly(other, NQ, BATCH);
    const int beta = (NQ + P.r.nP - 1) / P.r.nP;
    lr_poly *few = poly(q, NQ + P.r.nP, 2 * beta - 1), *thin = poly(q, NQ + P.r.nP - 1, 2 * beta);      // key images that are too small
    Outs o = outputs(P, S, BATCH, false), ob = Outs();
    for (int k = 0; k < S.n(); ++k) {
        ob.c0.push_back(poly(q, NQ, P.max_batch + 1));
        ob.c1.push_back(poly(q, NQ, P.max_batch + 1));
    }
    const lr_ckks_basis_product *p = S.p.data();
    const uint64_t *mult = S.mult.data(), *add = S.add.data();
    lr_poly *const *o0 = o.c0.data(), *const *o1 = o.c1.data();
    const int n = S.n();

    // LR_ERR_ARG, the header's order
    REFUSED(lr_ckks_power_basis(nullptr, n, p, mult, add, NQ, top, c0, c1, P.key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, nullptr, c1, P.key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, c0, nullptr, P.key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, c0, c1, nullptr, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_power_basis(pl, -1, p, mult, add, NQ, top, c0, c1, P.key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_power_basis(pl, n, nullptr, mult, add, NQ, top, c0, c1, P.key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_power_basis(pl, n, p, nullptr, add, NQ, top, c0, c1, P.key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_power_basis(pl, n, p, mult, nullptr, NQ, top, c0, c1, P.key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, c0, c1, P.key, nullptr, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, c0, c1, P.key, o0, nullptr), LR_ERR_ARG);
    {
        std::vector<lr_poly *> holed = o.c0;
        holed[1] = nullptr;
        REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, c0, c1, P.key, holed.data(), o1), LR_ERR_ARG);
        REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, c0, c1, P.key, o0, holed.data()), LR_ERR_ARG);
    }
    REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, top, top, c0, c1, P.key, o0, o1), LR_ERR_ARG);            // row_words below c1_level + 1
    {
        // a schedule that is not self-consistent, one field at a time
        auto broken = [&](int k, void (*spoil)(lr_ckks_basis_product &)) {
            std::vector<lr_ckks_basis_product> v = S.p;
            spoil(v[k]);
            REFUSED(lr_ckks_power_basis(pl, n, v.data(), mult, add, NQ, top, c0, c1, P.key, o0, o1), LR_ERR_ARG);
        };
        broken(1, [](lr_ckks_basis_product &x) { x.a = 9; });                       // an operand that is no product
        broken(0, [](lr_ckks_basis_product &x) { x.a = 3; });                       // ... that comes later
        broken(2, [](lr_ckks_basis_product &x) { x.layer = 1; });                   // ... of the same layer
        broken(1, [](lr_ckks_basis_product &x) { x.mul_level += 1; });
        broken(1, [](lr_ckks_basis_product &x) { x.mul_level -= 1; x.level_after -= 1; });
        broken(0, [](lr_ckks_basis_product &x) { x.tail = 3; });
        broken(0, [](lr_ckks_basis_product &x) { x.tail = -1; });
        broken(1, [](lr_ckks_basis_product &x) { x.mult_side = 3; });
        broken(0, [](lr_ckks_basis_product &x) { x.n_rescales = x.mul_level + 1; x.level_after = -1; });
        broken(0, [](lr_ckks_basis_product &x) { x.n_rescales = -1; x.level_after = x.mul_level + 1; });
        broken(0, [](lr_ckks_basis_product &x) { x.level_after += 1; });              // would read staging rows that the division dropped
        broken(0, [](lr_ckks_basis_product &x) { x.n = 1; });
        broken(2, [](lr_ckks_basis_product &x) { x.n = 2; });                       // listed twice
        broken(0, [](lr_ckks_basis_product &x) { x.tail = 1; });                    // C[2] has c == 0: no subtrahend
    }
    {
        std::vector<lr_poly *> twice = o.c0;
        twice[2] = twice[0];
        REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, c0, c1, P.key, twice.data(), o1), LR_ERR_ARG);
        twice = o.c1;
        twice[1] = o.c0[1];
        REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, c0, c1, P.key, o0, twice.data()), LR_ERR_ARG);
        twice = o.c0;
        twice[2] = c1;
        REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, c0, c1, P.key, twice.data(), o1), LR_ERR_ARG);   // an output over C[1]
    }
    // LR_ERR_SHAPE
    REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, big0, big1, P.key, ob.c0.data(), ob.c1.data()), LR_ERR_SHAPE);   // beyond max_batch
    REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, top, top, big0, big1, P.key, ob.c0.data(), ob.c1.data()), LR_ERR_ARG);    // two reasons: the argument checks first
    REFUSED(lr_ckks_power_basis(pl, 0, nullptr, nullptr, nullptr, NQ, -1, c0, c1, P.key, nullptr, nullptr), LR_ERR_SHAPE);     // level out of range
    {
        lr_ckks_basis_product high{};
        high.n = 2; high.a = high.b = 1; high.mul_level = high.level_after = NQ; high.layer = 1;
        REFUSED(lr_ckks_power_basis(pl, 1, &high, mult, add, NQ + 1, NQ, c0, c1, P.key, o0, o1), LR_ERR_SHAPE);
    }
    REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, foreign, c1, P.key, o0, o1), LR_ERR_SHAPE);       // another degree
    REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, c0, narrow, P.key, o0, o1), LR_ERR_SHAPE);        // fewer limbs than c1_level + 1
    {
        std::vector<lr_poly *> odd = o.c1;
        odd[1] = three;
        REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, c0, c1, P.key, o0, odd.data()), LR_ERR_SHAPE);   // another batch
        odd[1] = narrow;
        REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, c0, c1, P.key, o0, odd.data()), LR_ERR_SHAPE);   // fewer limbs than level_after + 1
        lr_poly *strided = poly(q, NQ + 1, BATCH);
        odd[1] = strided;
        REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, c0, c1, P.key, o0, odd.data()), LR_ERR_SHAPE);   // the pair's strides differ
        OK(lr_poly_free(strided));
    }
    REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, c0, c1, few, o0, o1), LR_ERR_SHAPE);
    REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, c0, c1, thin, o0, o1), LR_ERR_SHAPE);
    RUN(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, c0, c1, P.key, o0, o1));                               // and the call itself: accepted

    // the two contexts on different streams: a pipeline over both refuses
    hipStream_t s = nullptr;
    CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess);
    OK(lr_context_set_stream(q, s));
    REFUSED(lr_ckks_power_basis(pl, n, p, mult, add, NQ, top, c0, c1, P.key, o0, o1), LR_ERR_ARG);
    OK(lr_context_set_stream(q, nullptr));
    CHECK(hipStreamDestroy(s) == hipSuccess);

    // the schedule's own refusals: the code, nothing written
    {
        const uint32_t t[3] = {2, 3, 4}, zero[2] = {2, 0};
        const uint64_t even[NQ] = {Q5[0], Q5[1] + 1, Q5[2], Q5[3], Q5[4]};
        lr_ckks_basis_product out[3];
        uint64_t m[3 * NQ], a[3 * NQ];
        int count = -7;
        const double d = 1099511627776.0;
        auto untouched = [&] { return count == -7; };
        REFUSED(lr_ckks_power_basis_schedule(nullptr, NQ, d, 1, top, d, 3, t, 3, &count, out, m, a), LR_ERR_ARG);
        REFUSED(lr_ckks_power_basis_schedule(Q5, NQ, d, 1, top, d, 3, t, 3, nullptr, out, m, a), LR_ERR_ARG);
        REFUSED(lr_ckks_power_basis_schedule(Q5, NQ, d, 1, top, d, 3, nullptr, 3, &count, out, m, a), LR_ERR_ARG);
        REFUSED(lr_ckks_power_basis_schedule(Q5, NQ, d, 1, top, d, 3, t, 3, &count, nullptr, m, a), LR_ERR_ARG);
        REFUSED(lr_ckks_power_basis_schedule(Q5, NQ, d, 1, NQ, d, 3, t, 3, &count, out, m, a), LR_ERR_ARG);
        REFUSED(lr_ckks_power_basis_schedule(Q5, NQ, d, 1, top, d, 2, zero, 3, &count, out, m, a), LR_ERR_ARG);
        REFUSED(lr_ckks_power_basis_schedule(even, NQ, d, 1, top, d, 3, t, 3, &count, out, m, a), LR_ERR_ARG);
        REFUSED(lr_ckks_power_basis_schedule(Q5, NQ, 0.0, 1, top, d, 3, t, 3, &count, out, m, a), LR_ERR_ARG);
        REFUSED(lr_ckks_power_basis_schedule(Q5, NQ, d, 1, top, 1e200, 3, t, 3, &count, out, m, a), LR_ERR_ARG);
        CHECK(untouched());
        REFUSED(lr_ckks_power_basis_schedule(Q5, NQ, d, 1, top, d, 3, t, 2, &count, out, m, a), LR_ERR_ARG);
        CHECK(count == 3);
    }
    for (lr_poly *x : {c0, c1, narrow, three, big0, big1, foreign, few, thin}) OK(lr_poly_free(x));
    o.free_all();
    ob.free_all();
    OK(lr_context_destroy(other));
}

// the call as the first on a fresh plan, small and then larger: every pool and table slot it uses is allocated, and then grown, by this very call
static void cold(const Plan &P, const lr_options &opt, const std::vector<Sched> &all) {
    for (size_t first : {(size_t)2, (size_t)0, (size_t)4}) {
        Plan F = P;
        OK(lr_ckks_plan_create_ex(P.q, P.p, P.max_batch, &opt, &F.pl));
        run(F, all[first], 1, true);
        run(F, all[0], BATCH, true);
        OK(lr_ckks_plan_destroy(F.pl));
    }
}

int main() {
    const std::vector<Sched> all = schedules();
    for (const Ring &r : kRings) {
        for (int v = 0; v < 2; ++v) {
            lr_options opt;
            OK(lr_options_init(&opt));
            if (v == 1) opt.no_epilogue = 1;
            for (int max_batch : {BATCH, 2 * BATCH, 8 * BATCH}) {
                Plan P = make(r, opt, max_batch);
                const int fail_before = g_fail.load();
                for (const Sched &S : all) run(P, S, BATCH, true);
                run(P, all[0], 1, true);
                if (max_batch == 8 * BATCH) run(P, all[4], 8, true);      // the widest chunk a pair, at a batch of 8: product by product
                tensor_count(P);
                if (max_batch == 2 * BATCH) {
                    refusals(P);
                    cold(P, opt, all);
                }
                if (g_fail.load() != fail_before) std::fprintf(stderr, "... at N = 2^%d, variant %d, max_batch %d\n", r.logn, v, max_batch);
                drop(P);
            }
        }
    }
    CHECK(lr::g_ckks_basis_tail_launches.load() > 0 && lr::g_combine_launches.load() > 0);
    // two plans on two threads, each over its own contexts
    {
        lr_options opt;
        OK(lr_options_init(&opt));
        Plan A = make(kRings[0], opt, 2 * BATCH), B = make(kRings[3], opt, 2 * BATCH);
        std::thread ta([&] { for (const Sched &S : all) run(A, S, BATCH, false); });
        std::thread tb([&] { for (const Sched &S : all) run(B, S, BATCH, false); });
        ta.join();
        tb.join();
        drop(A);
        drop(B);
    }
    return driver_end(ALLOCATIONS | EVENTS, g_refusals, "ckks_basis: calls %d, refusals %d, tail launches %llu, tail products %llu, combine launches %llu", g_calls.load(),
                g_refusals.load(), lr::g_ckks_basis_tail_launches.load(), lr::g_ckks_basis_tail_products.load(), lr::g_combine_launches.load());
}
