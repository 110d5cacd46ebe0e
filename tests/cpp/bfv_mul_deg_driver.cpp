// BFV Mul's host side under AddressSanitizer + UBSan (tests/test_host_bfv_mul_deg_sanitizers.py): the REAL host code -- lr_abi_*.cpp (the one
// tensorAndRescale pipeline of lr_abi_bfv.cpp behind lr_bfv_mul and lr_bfv_mul_deg), lr_host.hpp, lr_precompute.cpp -- compiled with g++
// against the host-only HIP stand-in and the recording launch stubs of tests/cpp/hipstub/, which touch the first and the last word of every
// row a kernel would read or write.  Every degree pair with 1 <= d0 + d1 <= 5 through lr_bfv_mul_deg, 1 x 1 through lr_bfv_mul as well, the
// 1 x 1 and 2 x 2 squarings, at batches on both sides of the gather threshold, with and without the gathered path and the extension
// epilogues, with operands wider than |Q| limbs, with outputs written over operands, and every refusal.
// Exit code 0 = every check held; a sanitizer report aborts the run.  Nothing here computes: parity is the GPU suite's business.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "driver_check.hpp"

namespace lr {
extern std::atomic<unsigned long long> g_stub_launches;
}


// Q: Qm's first four; QMul: P3's first two
static const int NQ = 4, MAXB = 130;
static const uint64_t N = 1 << 10;

struct Operands {
    std::vector<lr_poly *> a, b, o;
    void free_all() {
        for (auto *v : {&a, &b, &o})
            for (lr_poly *p : *v) lr_poly_free(p);
    }
};
// wide: the second operand's polys hold |Q| + 1 limbs (a poly stride other than the pools')
static Operands make(lr_context *q, int d0, int d1, int batch, bool wide) {
    Operands r;
    for (int i = 0; i <= d0; ++i) r.a.push_back(poly(q, NQ, batch));
    for (int j = 0; j <= d1; ++j) r.b.push_back(poly(q, wide ? NQ + 1 : NQ, batch));
    for (int k = 0; k <= d0 + d1; ++k) r.o.push_back(poly(q, NQ, batch));
    return r;
}
static int call(lr_bfv_plan *pl, const std::vector<lr_poly *> &a, const std::vector<lr_poly *> &b, const std::vector<lr_poly *> &o) {
    std::vector<const lr_poly *> ca(a.begin(), a.end()), cb(b.begin(), b.end());
    return lr_bfv_mul_deg(pl, ca.data(), (int)a.size() - 1, cb.data(), (int)b.size() - 1, o.data());
}
// degree 1 x degree 1 through the fixed-arity entry point
static int call_mul(lr_bfv_plan *pl, const std::vector<lr_poly *> &a, const std::vector<lr_poly *> &b, const std::vector<lr_poly *> &o) {
    return lr_bfv_mul(pl, a[0], a[1], b[0], b[1], o[0], o[1], o[2]);
}

int main() {
    lr_context *q = nullptr, *m = nullptr;
    OK(lr_context_create(N, Qm, NQ, 0, &q));
    OK(lr_context_create(N, P3, 2, 0, &m));
    int calls = 0, refusals = 0;
    for (int variant = 0; variant < 3; ++variant) {
        lr_options opt;
        OK(lr_options_init(&opt));
        opt.bfv_no_gather = variant == 1;
        opt.bfv_no_ext_epilogue = variant == 2;
        lr_bfv_plan *pl = nullptr;
        OK(lr_bfv_plan_create_ex(q, m, 65537, MAXB, &opt, &pl));
        // batch 1 and 3 are gathered for every pair (nin * batch * 4 limbs <= 1536); at 130 none is
        for (int batch : {1, 3, MAXB}) {
            for (int d0 = 0; d0 <= 5; ++d0)
                for (int d1 = 0; d0 + d1 <= 5; ++d1) {
                    if (d0 + d1 < 1) continue;
                    const bool wide = (d0 + d1 + batch) % 2 == 1;
                    Operands r = make(q, d0, d1, batch, wide);
                    const unsigned long long before = lr::g_stub_launches.load();
                    OK(call(pl, r.a, r.b, r.o));
                    CHECK(lr::g_stub_launches.load() > before);
                    ++calls;
                    if (d0 == d1) {                                       // the squaring case: the same handles
                        OK(call(pl, r.a, r.a, r.o));
                        ++calls;
                    }
                    // outputs over operands (bfv_test.go:478 writes the product of a ciphertext and a plaintext over the ciphertext)
                    std::vector<lr_poly *> alias = r.o;
                    for (int i = 0; i <= d0; ++i) alias[i] = r.a[i];
                    if (!wide) alias[d0 + d1] = r.b[d1];
                    OK(call(pl, r.a, r.b, alias));
                    ++calls;
                    if (d0 == 1 && d1 == 1) {                             // lr_bfv_mul's pointer packing: the same three calls
                        OK(call_mul(pl, r.a, r.b, r.o));
                        OK(call_mul(pl, r.a, r.a, r.o));
                        OK(call_mul(pl, r.a, r.b, alias));
                        calls += 3;
                    }
                    r.free_all();
                }
        }
        // refusals: no launch, an error code
        {
            Operands r = make(q, 2, 1, 2, false);
            const unsigned long long before = lr::g_stub_launches.load();
            std::vector<lr_poly *> seven(r.o);                            // 4 outputs of 2 x 1, and 3 more
            for (int k = 0; k < 3; ++k) seven.push_back(poly(q, NQ, 2));
            std::vector<lr_poly *> d3(r.a);
            d3.push_back(r.b[0]);
            CHECK(call(pl, d3, d3, seven) == LR_ERR_ARG);                                                              // 3 x 3: sum 6
            CHECK(call(pl, {r.a[0], r.a[1], r.a[2], r.b[0], r.b[1], r.o[0]}, {r.b[0], r.b[1]}, seven) == LR_ERR_ARG);  // 5 x 1
            CHECK(call(pl, {r.a[0]}, {r.b[0]}, {r.o[0]}) == LR_ERR_ARG);                                               // 0 x 0
            const lr_poly *one[1] = {r.a[0]};
            lr_poly *outs[2] = {r.o[0], r.o[1]};
            CHECK(lr_bfv_mul_deg(pl, one, -1, one, 1, outs) == LR_ERR_ARG);                                           // negative degree
            CHECK(call(pl, r.a, r.b, {r.o[0], r.o[1], r.o[2], r.o[1]}) == LR_ERR_ARG);                                 // duplicate outputs
            CHECK(call(pl, r.a, r.b, {r.o[0], r.o[1], r.o[2], nullptr}) == LR_ERR_ARG);                                // null output
            CHECK(call(pl, r.a, {r.b[0], nullptr}, r.o) == LR_ERR_ARG);                                                // null operand
            CHECK(lr_bfv_mul_deg(nullptr, one, 0, one, 1, outs) == LR_ERR_ARG);
            CHECK(lr_bfv_mul_deg(pl, nullptr, 0, one, 1, outs) == LR_ERR_ARG);
            CHECK(lr_bfv_mul_deg(pl, one, 0, one, 1, nullptr) == LR_ERR_ARG);
            lr_poly *narrow = poly(q, NQ - 1, 2), *other = poly(q, NQ, 3), *big = poly(q, NQ, MAXB + 1);
            CHECK(call(pl, r.a, {r.b[0], narrow}, r.o) == LR_ERR_SHAPE);                                               // too few limbs
            CHECK(call(pl, r.a, {r.b[0], other}, r.o) == LR_ERR_SHAPE);                                                // batch mismatch
            CHECK(call(pl, r.a, r.b, {r.o[0], r.o[1], r.o[2], other}) == LR_ERR_SHAPE);
            std::vector<lr_poly *> bigs{big, poly(q, NQ, MAXB + 1)}, bigo{poly(q, NQ, MAXB + 1), poly(q, NQ, MAXB + 1)};
            CHECK(call(pl, bigs, {bigs[0]}, bigo) == LR_ERR_SHAPE);                                                    // batch > max_batch
            CHECK(call_mul(pl, r.a, r.b, {r.o[0], r.o[1], r.o[0]}) == LR_ERR_ARG);                                     // lr_bfv_mul: duplicate outputs
            CHECK(lr::g_stub_launches.load() == before);
            refusals += 15;
            for (lr_poly *p : {seven[4], seven[5], seven[6], narrow, other, bigs[1], bigo[0], bigo[1]}) lr_poly_free(p);
            lr_poly_free(big);
            r.free_all();
        }
        OK(lr_bfv_plan_destroy(pl));
    }
    OK(lr_context_destroy(m));
    OK(lr_context_destroy(q));
    return driver_end(0, refusals, "bfv_mul_deg: calls %d, refusals %d", calls, refusals);
}
