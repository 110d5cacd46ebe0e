// The key switch's host side under AddressSanitizer + UBSan (tests/test_host_key_switch_sanitizers.py): the REAL host code -- lr_abi_*.cpp (the
// decomposition, the key inner product and the two ModDown tails of lr_abi_ckks.cpp, the digit shapes of lr_abi_bext.cpp), lr_host.hpp,
// lr_precompute.cpp -- compiled with g++ against the host-only HIP stand-in and the recording launch stubs of tests/cpp/hipstub/, which touch
// the first and the last word of every row a kernel would read or write.  lr_ckks_switch_keys, lr_ckks_mulrelin, lr_ckks_rotate,
// lr_ckks_rotate_hoisted (two rotations), lr_ckks_rescale, lr_bfv_switch_keys, lr_bfv_relinearize and lr_bfv_rotate (lr_abi_bfv_eval.cpp) over
//   * N = 2^12 (|Q| = 5, |P| = 3: digits of 3 + 2 limbs), 2^15 (|Q| = 5, |P| = 2: 2 + 2 + 1) and 2^16 (|Q| = 4, |P| = 2, the six primes there are:
//     the top-stage extensions, the staging buffers and the forks of a lone plan), every level from 0 to |Q| - 1 -- full digits, partial last
//     digits, single-limb digits, the trivial-copy branch;
//   * batches 1, 2 and 5, and once more with pair_max_workgroups and fork_below_workgroups lowered to 4 (both sides of each threshold);
//   * every launch-shape option of the plan;
//   * outputs written over operands and over each other where the entry point allows it (the paired launches' refusal side);
//   * each entry point as the first call on a fresh plan and then at a larger batch (its pools are allocated, then moved, by that call);
//   * each entry point's refusals: the code, and that nothing was launched;
//   * the same over the rings given on the command line ("logN |Q| |P| q.. p.." each: the test passes moduli at the limits of the admission
//     bounds -- Q and P just under 2^61 with one special prime, either side of 2^57, either side of 2^33).
// Exit code 0 = every check held; a sanitizer report aborts the run.  Nothing here computes: parity is the GPU suite's business.
#include <algorithm>
#include <cstdlib>
#include <deque>
#include <vector>

// a successful call here also launches something
#define RUN(x)                                                             \
    do {                                                                   \
        const unsigned long long before_ = lr::g_stub_launches.load();     \
        OK(x);                                                             \
        CHECK(lr::g_stub_launches.load() > before_);                       \
        ++g_calls;                                                         \
    } while (0)
#include "driver_check.hpp"

static const int MAXB = 5;

struct Ring {
    uint64_t N;
    const uint64_t *Q;
    int nQ;
    const uint64_t *P;
    int nP;
};
static const Ring kRings[3] = {{1 << 12, Q5, 5, P3, 3}, {1 << 15, Q5, 5, P3, 2}, {1 << 16, Q16, 4, P16, 2}};

static const int kVariants = 10;
static const char *set_variant(lr_options *o, int v) {
    switch (v) {
    case 0: return "default";
    case 1: o->no_pair = 1; return "no_pair";
    case 2: o->no_fork = 1; return "no_fork";
    case 3: o->no_ext_group = 1; return "no_ext_group";
    case 4: o->no_exttop = 1; return "no_exttop";
    case 5: o->no_exttop = 1; o->no_staging = 1; return "no_exttop+no_staging";
    case 6: o->no_invtop = 1; return "no_invtop";
    case 7: o->no_epilogue = 1; return "no_epilogue";
    case 8: o->keymac_narrow = 1; return "keymac_narrow";
    default: o->pair_max_workgroups = 4; o->fork_below_workgroups = 4; return "low thresholds";
    }
}

static uintptr_t address(const lr_poly *p) {
    void *d = nullptr;
    OK(lr_poly_info(p, nullptr, nullptr, nullptr, &d));
    return (uintptr_t)d;
}
static std::vector<lr_poly *> sorted_polys(lr_context *ctx, int limbs, int batch, int count) {
    std::vector<lr_poly *> v;
    for (int i = 0; i < count; ++i) v.push_back(poly(ctx, limbs, batch));
    std::sort(v.begin(), v.end(), [](const lr_poly *x, const lr_poly *y) { return address(x) < address(y); });
    return v;
}

struct Plan {
    Ring r;
    lr_context *q = nullptr, *p = nullptr;
    lr_ckks_plan *pl = nullptr;
    lr_poly *key = nullptr;
};

static int hoisted(const Plan &P, int level, lr_poly *c0, lr_poly *c1, lr_poly *const *o0, lr_poly *const *o1, int n_rot = 2) {
    const uint64_t gens[2] = {5, 25};
    const lr_poly *keys[2] = {P.key, P.key};
    return lr_ckks_rotate_hoisted(P.pl, level, c0, c1, n_rot, gens, keys, o0, o1);
}

// every entry point at one batch: the CKKS ones at every level, the BFV ones at the top level (they have no other)
static void calls(const Plan &P, int batch) {
    lr_context *q = P.q;
    const int nQ = P.r.nQ;
    // in ascending address order: a pair of outputs is then at a positive distance, whatever the allocator does (descending inputs and, below
    // N = 2^16, descending outputs are exercised further down)
    std::vector<lr_poly *> v = sorted_polys(q, nQ, batch, 8), w = sorted_polys(q, nQ + 1, batch, 2);      // w: another poly stride than the pools'
    lr_poly *a0 = v[0], *a1 = v[1], *b0 = v[2], *b1 = v[3], *o0 = v[4], *o1 = v[5], *h0 = v[6], *h1 = v[7], *wide0 = w[0], *wide1 = w[1];
    lr_poly *outs0[2] = {o0, h0}, *outs1[2] = {o1, h1};
    for (int level = 0; level < nQ; ++level) {
        RUN(lr_ckks_switch_keys(P.pl, level, a0, P.key, o0, o1));
        if (address(wide0) < address(o1)) RUN(lr_ckks_switch_keys(P.pl, level, a0, P.key, wide0, o1));       // outputs with different strides
        else RUN(lr_ckks_switch_keys(P.pl, level, a0, P.key, o1, wide0));
        RUN(lr_ckks_switch_keys(P.pl, level, a0, P.key, a0, o1));          // over the input
        RUN(lr_ckks_switch_keys(P.pl, level, a0, P.key, o0, o0));          // the same output twice: never one paired launch
        RUN(lr_ckks_mulrelin(P.pl, level, a0, a1, b0, b1, P.key, o0, o1));
        RUN(lr_ckks_mulrelin(P.pl, level, a0, a1, a0, a1, P.key, wide0, wide1));
        RUN(lr_ckks_mulrelin(P.pl, level, a0, a1, b0, b1, P.key, a0, a1));
        RUN(lr_ckks_mulrelin(P.pl, level, a0, a1, b0, b1, P.key, o0, o0));
        RUN(lr_ckks_rotate(P.pl, level, a0, a1, 5, P.key, o0, o1));
        RUN(lr_ckks_rotate(P.pl, level, a0, wide1, 25, P.key, wide0, wide1));
        RUN(lr_ckks_rotate(P.pl, level, a0, a1, 5, P.key, a0, a1));
        RUN(lr_ckks_rotate(P.pl, level, a0, a0, 5, P.key, o0, o1));        // the same component twice
        RUN(lr_ckks_rotate(P.pl, level, a1, a0, 5, P.key, o0, o1));        // components in descending address order
        RUN(lr_ckks_rotate(P.pl, level, a0, a1, 2 * P.r.N - 1, P.key, o0, o0));   // Conjugate's element; one output twice
        RUN(hoisted(P, level, a0, a1, outs0, outs1));
        RUN(hoisted(P, level, a0, a0, outs0, outs1));
        RUN(hoisted(P, level, a0, a1, outs0, outs1, 0));                   // no rotation: the decomposition alone
        if (P.r.N < (1u << 16)) {
            // outputs in descending address order: the pair's stride is negative (at N = 2^16 without the top-stage extension the transform
            // that carries the epilogue refuses such a launch, see component_pair in lr_host.hpp: not asked for here)
            RUN(lr_ckks_switch_keys(P.pl, level, a0, P.key, o1, o0));
            RUN(lr_ckks_mulrelin(P.pl, level, a0, a1, b0, b1, P.key, o1, o0));
            RUN(lr_ckks_rotate(P.pl, level, a0, a1, 5, P.key, o1, o0));
        }
        if (level > 0) {
            // (rescale drops a limb: the handles get their limb count back)
            lr_poly *r0 = poly(q, level + 1, batch), *r1 = poly(q, level + 1, batch), *both = poly(q, level + 1, 2 * batch);
            RUN(lr_ckks_rescale(P.pl, r0, r1));
            OK(lr_poly_set_limbs(r0, level + 1));
            OK(lr_poly_set_limbs(r1, level + 1));
            RUN(lr_ckks_rescale(P.pl, r1, r0));
            OK(lr_poly_set_limbs(r0, level + 1));
            if (level > 1) RUN(lr_ckks_rescale(P.pl, r0, r0));             // the same poly twice: two divisions in a row
            void *base = nullptr;
            OK(lr_poly_info(both, nullptr, nullptr, nullptr, &base));
            lr_poly *lo = nullptr, *hi = nullptr;                          // two batches laid out back to back
            OK(lr_poly_wrap(q, base, level + 1, batch, &lo));
            OK(lr_poly_wrap(q, (uint64_t *)base + (size_t)batch * (level + 1) * P.r.N, level + 1, batch, &hi));
            RUN(lr_ckks_rescale(P.pl, lo, hi));
            for (lr_poly *x : {r0, r1, both, lo, hi}) OK(lr_poly_free(x));
        }
    }
    RUN(lr_bfv_switch_keys(P.pl, a0, P.key, o0, o1));
    RUN(lr_bfv_switch_keys(P.pl, a0, P.key, wide0, o1));
    RUN(lr_bfv_relinearize(P.pl, a0, a1, b0, P.key, o0, o1));
    RUN(lr_bfv_relinearize(P.pl, a0, a1, b0, P.key, a0, a1));              // the reference's own use: over c0 / c1
    RUN(lr_bfv_relinearize(P.pl, a0, a1, b0, P.key, a1, a0));              // crosswise: the paired addition must refuse
    RUN(lr_bfv_relinearize(P.pl, a0, a0, b0, P.key, o0, o1));
    RUN(lr_bfv_relinearize(P.pl, wide0, a1, b0, P.key, o0, wide1));
    RUN(lr_bfv_rotate(P.pl, a0, a1, 5, P.key, o0, o1));
    RUN(lr_bfv_rotate(P.pl, a0, a1, 2 * P.r.N - 1, P.key, a0, a1));        // RotateRows' element, in place
    RUN(lr_bfv_rotate(P.pl, a0, a0, 5, P.key, o0, o1));
    RUN(lr_bfv_rotate(P.pl, a1, a0, 5, P.key, wide0, o1));
    for (lr_poly *x : {a0, a1, b0, b1, o0, o1, h0, h1, wide0, wide1}) OK(lr_poly_free(x));
}

static void refusals(const Plan &P) {
    lr_context *q = P.q;
    lr_ckks_plan *pl = P.pl;
    const int nQ = P.r.nQ, top = nQ - 1;
    lr_poly *a0 = poly(q, nQ, 2), *a1 = poly(q, nQ, 2), *b0 = poly(q, nQ, 2), *o0 = poly(q, nQ, 2), *o1 = poly(q, nQ, 2), *h0 = poly(q, nQ, 2), *h1 = poly(q, nQ, 2);
    lr_poly *narrow = poly(q, nQ - 1, 2), *three = poly(q, nQ, 3), *wide = poly(q, nQ + 1, 2), *small_key = poly(q, nQ + P.r.nP, 1);
    lr_poly *big[5];
    for (lr_poly *&x : big) x = poly(q, nQ, MAXB + 1);
    lr_poly *outs0[2] = {o0, h0}, *outs1[2] = {o1, h1};
    const lr_poly *key = P.key;

    REFUSED(lr_ckks_switch_keys(nullptr, top, a0, key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_switch_keys(pl, top, a0, nullptr, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_switch_keys(pl, top, a0, key, o0, nullptr), LR_ERR_ARG);
    REFUSED(lr_ckks_switch_keys(pl, -1, a0, key, o0, o1), LR_ERR_SHAPE);
    REFUSED(lr_ckks_switch_keys(pl, nQ, a0, key, o0, o1), LR_ERR_SHAPE);
    REFUSED(lr_ckks_switch_keys(pl, top, big[0], key, big[1], big[2]), LR_ERR_SHAPE);
    REFUSED(lr_ckks_switch_keys(pl, top, a0, key, narrow, o1), LR_ERR_SHAPE);
    REFUSED(lr_ckks_switch_keys(pl, top, a0, key, o0, three), LR_ERR_SHAPE);
    OK(lr_ckks_switch_keys(pl, top - 1, a0, key, narrow, o1));                       // (enough limbs one level down)
    CHECK(lr_ckks_switch_keys(pl, top, a0, small_key, o0, o1) == LR_ERR_SHAPE);      // found when the inner product is reached
    ++g_refusals;

    REFUSED(lr_ckks_mulrelin(nullptr, top, a0, a1, a0, a1, key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_mulrelin(pl, top, a0, a1, nullptr, a1, key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_mulrelin(pl, nQ, a0, a1, a0, a1, key, o0, o1), LR_ERR_SHAPE);
    REFUSED(lr_ckks_mulrelin(pl, top, big[0], big[1], big[0], big[1], key, big[2], big[3]), LR_ERR_SHAPE);
    REFUSED(lr_ckks_mulrelin(pl, top, a0, a1, a0, narrow, key, o0, o1), LR_ERR_SHAPE);
    REFUSED(lr_ckks_mulrelin(pl, top, a0, a1, a0, a1, key, three, o1), LR_ERR_SHAPE);
    REFUSED(lr_ckks_mulrelin(pl, top, a0, a1, a0, a1, key, o0, wide), LR_ERR_SHAPE);            // outputs share their stride

    REFUSED(lr_ckks_rotate(nullptr, top, a0, a1, 5, key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_rotate(pl, top, a0, a1, 5, nullptr, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_rotate(pl, -1, a0, a1, 5, key, o0, o1), LR_ERR_SHAPE);
    REFUSED(lr_ckks_rotate(pl, top, big[0], big[1], 5, key, big[2], big[3]), LR_ERR_SHAPE);
    REFUSED(lr_ckks_rotate(pl, top, a0, narrow, 5, key, o0, o1), LR_ERR_SHAPE);
    REFUSED(lr_ckks_rotate(pl, top, a0, a1, 5, key, o0, three), LR_ERR_SHAPE);
    REFUSED(lr_ckks_rotate(pl, top, a0, a1, 5, key, wide, o1), LR_ERR_SHAPE);

    REFUSED(hoisted(P, top, nullptr, a1, outs0, outs1), LR_ERR_ARG);
    REFUSED(hoisted(P, top, a0, a1, nullptr, outs1), LR_ERR_ARG);
    REFUSED(hoisted(P, top, a0, a1, outs0, outs1, -1), LR_ERR_ARG);
    REFUSED(hoisted(P, nQ, a0, a1, outs0, outs1), LR_ERR_SHAPE);
    REFUSED(hoisted(P, top, big[0], big[1], outs0, outs1), LR_ERR_SHAPE);
    REFUSED(hoisted(P, top, a0, narrow, outs0, outs1), LR_ERR_SHAPE);
    {
        lr_poly *bad0[2] = {o0, nullptr}, *bad1[2] = {o1, three}, *bad2[2] = {o1, wide}, *bad3[2] = {o1, a1};
        REFUSED(hoisted(P, top, a0, a1, bad0, outs1), LR_ERR_ARG);
        REFUSED(hoisted(P, top, a0, a1, outs0, bad1), LR_ERR_SHAPE);
        REFUSED(hoisted(P, top, a0, a1, outs0, bad2), LR_ERR_SHAPE);
        REFUSED(hoisted(P, top, a0, a1, outs0, bad3), LR_ERR_ARG);                   // not in place
    }

    REFUSED(lr_bfv_switch_keys(nullptr, a0, key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_switch_keys(pl, a0, key, nullptr, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_switch_keys(pl, a0, key, a0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_switch_keys(pl, a0, key, o0, o0), LR_ERR_ARG);
    REFUSED(lr_bfv_switch_keys(pl, a0, key, narrow, o1), LR_ERR_SHAPE);
    REFUSED(lr_bfv_switch_keys(pl, a0, key, o0, three), LR_ERR_SHAPE);
    REFUSED(lr_bfv_switch_keys(pl, big[0], key, big[1], big[2]), LR_ERR_SHAPE);
    REFUSED(lr_bfv_switch_keys(pl, big[0], key, big[1], big[1]), LR_ERR_ARG);        // two reasons: distinctness is asked first
    REFUSED(lr_bfv_switch_keys(pl, big[0], key, narrow, big[2]), LR_ERR_SHAPE);

    REFUSED(lr_bfv_relinearize(nullptr, a0, a1, b0, key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_relinearize(pl, a0, a1, b0, nullptr, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_relinearize(pl, a0, narrow, b0, key, o0, o1), LR_ERR_SHAPE);
    REFUSED(lr_bfv_relinearize(pl, a0, a1, b0, key, three, o1), LR_ERR_SHAPE);
    REFUSED(lr_bfv_relinearize(pl, a0, a1, b0, key, o0, o0), LR_ERR_ARG);
    REFUSED(lr_bfv_relinearize(pl, a0, a1, b0, key, b0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_relinearize(pl, three, a1, b0, key, o0, o0), LR_ERR_SHAPE);       // two reasons: the shapes are asked first
    REFUSED(lr_bfv_relinearize(pl, big[0], big[1], big[2], key, big[3], big[4]), LR_ERR_SHAPE);
    REFUSED(lr_bfv_relinearize(pl, big[0], big[1], big[2], key, big[3], big[3]), LR_ERR_ARG);   // ... and max_batch last

    REFUSED(lr_bfv_rotate(nullptr, a0, a1, 5, key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_rotate(pl, a0, a1, 5, key, o0, nullptr), LR_ERR_ARG);
    REFUSED(lr_bfv_rotate(pl, big[0], big[1], 5, key, big[2], big[3]), LR_ERR_SHAPE);
    REFUSED(lr_bfv_rotate(pl, big[0], big[1], 5, key, big[2], big[2]), LR_ERR_SHAPE);            // two reasons: max_batch is asked first
    REFUSED(lr_bfv_rotate(pl, a0, narrow, 5, key, o0, o1), LR_ERR_SHAPE);
    REFUSED(lr_bfv_rotate(pl, a0, a1, 5, key, three, o1), LR_ERR_SHAPE);
    REFUSED(lr_bfv_rotate(pl, a0, a1, 5, key, o0, o0), LR_ERR_ARG);
    REFUSED(lr_bfv_rotate(pl, three, a1, 5, key, o0, o0), LR_ERR_SHAPE);

    REFUSED(lr_ckks_rescale(pl, nullptr, a1), LR_ERR_ARG);
    REFUSED(lr_ckks_rescale(nullptr, a0, a1), LR_ERR_ARG);

    // the two contexts on different streams: every pipeline over both refuses
    hipStream_t s = nullptr;
    CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess);
    OK(lr_context_set_stream(q, s));
    REFUSED(lr_ckks_switch_keys(pl, top, a0, key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_mulrelin(pl, top, a0, a1, a0, a1, key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_rotate(pl, top, a0, a1, 5, key, o0, o1), LR_ERR_ARG);
    REFUSED(hoisted(P, top, a0, a1, outs0, outs1), LR_ERR_ARG);
    REFUSED(lr_bfv_switch_keys(pl, a0, key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_relinearize(pl, a0, a1, b0, key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_bfv_rotate(pl, a0, a1, 5, key, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_switch_keys(pl, top, a0, key, o0, three), LR_ERR_SHAPE);         // two reasons: the shapes are asked first
    OK(lr_context_set_stream(q, nullptr));
    CHECK(hipStreamDestroy(s) == hipSuccess);

    for (lr_poly *x : {a0, a1, b0, o0, o1, h0, h1, narrow, three, wide, small_key}) OK(lr_poly_free(x));
    for (lr_poly *x : big) OK(lr_poly_free(x));
}

// each entry point as the first call on a fresh plan, then at a larger batch: every pool it uses is allocated, and then moved, by this very call
static void cold(const Ring &r, const lr_options &opt, lr_context *q, lr_context *p, const lr_poly *key) {
    for (int entry = 0; entry < 7; ++entry) {
        Plan P;
        P.r = r;
        P.q = q;
        P.p = p;
        P.key = const_cast<lr_poly *>(key);
        OK(lr_ckks_plan_create_ex(q, p, MAXB, &opt, &P.pl));
        for (int batch : {2, MAXB}) {
            std::vector<lr_poly *> v = sorted_polys(q, r.nQ, batch, 7);
            lr_poly *outs0[2] = {v[3], v[5]}, *outs1[2] = {v[4], v[6]};
            const int top = r.nQ - 1;
            switch (entry) {
            case 0: RUN(lr_ckks_switch_keys(P.pl, top, v[0], key, v[3], v[4])); break;
            case 1: RUN(lr_ckks_mulrelin(P.pl, top, v[0], v[1], v[0], v[2], key, v[3], v[4])); break;
            case 2: RUN(lr_ckks_rotate(P.pl, top, v[0], v[1], 5, key, v[3], v[4])); break;
            case 3: RUN(hoisted(P, top, v[0], v[1], outs0, outs1)); break;
            case 4: RUN(lr_bfv_switch_keys(P.pl, v[0], key, v[3], v[4])); break;
            case 5: RUN(lr_bfv_relinearize(P.pl, v[0], v[1], v[2], key, v[3], v[4])); break;
            default: RUN(lr_bfv_rotate(P.pl, v[0], v[1], 5, key, v[3], v[4])); break;
            }
            for (lr_poly *x : v) OK(lr_poly_free(x));
        }
        OK(lr_ckks_plan_destroy(P.pl));
    }
}

int main(int argc, char **argv) {
    unsigned long long forks16 = 0, forks_other = 0, grouped = 0;
    std::vector<Ring> rings(kRings, kRings + 3);
    std::deque<std::vector<uint64_t>> extra;                               // (a deque: the rings keep pointers into its elements)
    for (int a = 1; a + 2 < argc;) {
        const int logn = std::atoi(argv[a]), nq = std::atoi(argv[a + 1]), np = std::atoi(argv[a + 2]);
        CHECK(a + 3 + nq + np <= argc);
        extra.emplace_back();
        for (int i = 0; i < nq + np; ++i) extra.back().push_back(std::strtoull(argv[a + 3 + i], nullptr, 10));
        rings.push_back(Ring{(uint64_t)1 << logn, extra.back().data(), nq, extra.back().data() + nq, np});
        a += 3 + nq + np;
    }
    for (const Ring &r : rings) {
        for (int v = 0; v < kVariants; ++v) {
            lr_options opt;
            OK(lr_options_init(&opt));
            const char *name = set_variant(&opt, v);
            Plan P;
            P.r = r;
            OK(lr_context_create_ex(r.N, r.Q, r.nQ, 0, &opt, &P.q));
            OK(lr_context_create_ex(r.N, r.P, r.nP, 0, &opt, &P.p));
            OK(lr_ckks_plan_create_ex(P.q, P.p, MAXB, &opt, &P.pl));
            const int beta = (r.nQ + r.nP - 1) / r.nP;
            P.key = poly(P.q, r.nQ + r.nP, 2 * beta);
            const int fail_before = g_fail;
            for (int batch : {1, 2, MAXB}) calls(P, batch);
            refusals(P);
            uint64_t f = 0, g = 0;
            OK(lr_ckks_plan_stats(P.pl, &f, &g));
            (r.N == (1u << 16) ? forks16 : forks_other) += f;
            grouped += g;
            if (v == 2) CHECK(f == 0);
            if (v == 3) CHECK(g == 0);
            if (g_fail != fail_before) std::fprintf(stderr, "... at N = %llu, %s\n", (unsigned long long)r.N, name);
            OK(lr_ckks_plan_destroy(P.pl));
            cold(r, opt, P.q, P.p, P.key);
            OK(lr_poly_free(P.key));
            OK(lr_context_destroy(P.q));
            OK(lr_context_destroy(P.p));
        }
    }
    CHECK(forks16 > 0 && forks_other == 0 && grouped > 0);                // the lone plan forks at N = 2^16 only; the digits' extensions are grouped
    return driver_end(ALLOCATIONS, g_refusals, "key_switch: calls %d, refusals %d, forks %llu, grouped extensions %llu", g_calls.load(), g_refusals.load(), forks16, grouped);
}
