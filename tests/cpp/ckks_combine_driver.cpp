// The host side of the CKKS combine call under AddressSanitizer + UBSan and under ThreadSanitizer
// (tests/test_host_ckks_combine_sanitizers.py): the REAL host code -- lr_abi_*.cpp (lr_abi_ckks_eval.cpp, lr_abi_ckks_scalar.cpp), lr_host.hpp,
// lr_precompute.cpp -- compiled with g++ against the host-only HIP stand-in and the recording launch stubs of tests/cpp/hipstub/; the
// stand-in of the pass's launcher keeps every launch and touches the first and the last word of every row a kernel would read or write.  Every refusal in the stated order with the message its caller reads; for every degree pair with b
// present and absent, every flag combination and every receiver identity what the one launch carries -- addresses, strides (0 for an
// operand of batch 1), degrees, flags and the six words of every limb -- on polys whose members lie apart by more than their limbs and at
// a level below their limb count; the constants function on two threads.  Exit code 0 = every check held; a sanitizer report aborts the
// run.  Nothing here computes on polys: parity is the GPU suite's business.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "lr_device.hpp"

namespace lr {
struct CombineRecord {
    CombineLaunch L;
    int limbs, batch;
};
extern std::atomic<unsigned long long> g_stub_launches, g_combine_launches;
extern std::mutex g_combine_mu;
extern std::vector<CombineRecord> g_combine_log;
}  // namespace lr

#define REFUSED REFUSED_MSG_NO_LAUNCH      // here a refusal launches nothing of any kind and is logged with its message
#include "driver_check.hpp"

static std::vector<lr::CombineRecord> take_log() {
    std::lock_guard<std::mutex> lock(lr::g_combine_mu);
    std::vector<lr::CombineRecord> out;
    out.swap(lr::g_combine_log);
    return out;
}

static uint64_t *device_ptr(const lr_poly *p) {
    uint64_t *d = nullptr;
    OK(lr_poly_info(p, nullptr, nullptr, nullptr, (void **)&d));
    return d;
}

// the launch of one accepted call against what the contract says it carries.  receiver: 0 fresh polys, 1 a, 2 b, 3 a is b is the
// receiver; shared: 0 none, 1 a has batch 1, 2 b has batch 1
static void one_call(lr_context *ctx, uint64_t N, int nq, int level, int op, int deg_a, int deg_b, unsigned flags, int batch, int receiver, int shared,
                     bool strided) {
    const int L1 = level + 1, comps = (deg_a > deg_b ? deg_a : deg_b) + 1;
    const bool double_a = flags & 1u, mult_a = flags & 2u, mult_b = (flags & 4u) && deg_b >= 0, with_add = flags & 8u;
    const int limbs = L1 + (level + 1 < nq ? 1 : 0);
    std::vector<void *> raw;
    std::vector<lr_poly *> own;
    const auto make = [&](int members) -> lr_poly * {
        lr_poly *p = nullptr;
        if (!strided) {
            p = poly(ctx, limbs, members);
        } else {        // members two limbs further apart (a view into a larger poly), exactly what the view spans
            const long long stride = (long long)(limbs + 2) * (long long)N;
            void *d = nullptr;
            CHECK(hipMalloc(&d, (size_t)((members - 1) * stride + (long long)limbs * (long long)N) * sizeof(uint64_t)) == hipSuccess);
            raw.push_back(d);
            OK(lr_poly_wrap_strided(ctx, d, limbs, members, stride, &p));
        }
        own.push_back(p);
        return p;
    };
    const long long full_stride = (long long)(limbs + (strided ? 2 : 0)) * (long long)N;
    std::vector<const lr_poly *> a, b;
    std::vector<lr_poly *> out;
    for (int u = 0; u <= deg_a; ++u) a.push_back(make(shared == 1 ? 1 : batch));
    if (receiver == 3) b = a;
    else
        for (int u = 0; u <= deg_b; ++u) b.push_back(make(shared == 2 ? 1 : batch));
    for (int u = 0; u < comps; ++u) {
        const std::vector<const lr_poly *> &src = receiver == 2 ? b : a;
        out.push_back(receiver != 0 && u < (int)src.size() ? const_cast<lr_poly *>(src[u]) : make(batch));
    }
    // exactly level + 1 words each, every one distinct
    std::vector<uint64_t> w[6];
    for (int j = 0; j < 6; ++j) {
        w[j].resize((size_t)L1);
        for (int i = 0; i < L1; ++i) w[j][i] = 1000000ull * (uint64_t)(j + 1) + (uint64_t)i;
    }
    (void)take_log();
    OK(lr_ckks_combine(ctx, op, level, deg_a, a.data(), deg_b, deg_b >= 0 ? b.data() : nullptr, double_a ? 1 : 0, mult_a ? w[0].data() : nullptr,
                       mult_a ? w[1].data() : nullptr, mult_b ? w[2].data() : nullptr, mult_b ? w[3].data() : nullptr, with_add ? w[4].data() : nullptr,
                       with_add ? w[5].data() : nullptr, out.data()));
    const std::vector<lr::CombineRecord> log = take_log();
    CHECK(log.size() == 1);                              // every limb's words fit one launch
    if (log.size() == 1) {
        const lr::CombineRecord &r = log[0];
        const lr::CombineLaunch &L = r.L;
        CHECK(r.batch == batch && r.limbs == L1 && L.n == (int)N && L.op == op && L.deg_a == deg_a && L.deg_b == (deg_b >= 0 ? deg_b : -1));
        CHECK(L.double_a == (int)double_a && L.mult_a == (int)mult_a && L.mult_b == (int)mult_b && L.has_add == (int)with_add);
        const auto stride_of = [&](int members) { return members == 1 && batch > 1 ? 0ll : full_stride; };
        for (int u = 0; u <= deg_a; ++u) CHECK(L.a[u] == device_ptr(a[u]) && L.a_stride[u] == stride_of(shared == 1 ? 1 : batch));
        for (int u = 0; u <= deg_b; ++u) CHECK(L.b[u] == device_ptr(b[u]) && L.b_stride[u] == stride_of(shared == 2 ? 1 : batch));
        for (int u = 0; u < comps; ++u) CHECK(L.out[u] == device_ptr(out[u]) && L.out_stride[u] == full_stride);
        for (int u = deg_a + 1; u < lr::kCombineComps; ++u) CHECK(L.a[u] == nullptr);
        for (int u = deg_b + 1; u < lr::kCombineComps; ++u) CHECK(L.b[u] == nullptr);
        for (int i = 0; i < L1; ++i) {
            const uint64_t *k = L.k + (size_t)i * lr::kCombineLimbWords;
            const bool on[6] = {mult_a, mult_a, mult_b, mult_b, with_add, with_add};
            for (int j = 0; j < 6; ++j) CHECK(k[j] == (on[j] ? w[j][i] : 0));
        }
    }
    OK(lr_context_sync(ctx));
    for (lr_poly *p : own) lr_poly_free(p);
    for (void *d : raw) (void)hipFree(d);
}

static int refusals() {
    const uint64_t N = 16;
    const int nq = 3, top = 2;
    lr_context *ctx = nullptr, *tiny = nullptr, *big = nullptr;
    OK(lr_context_create(N, M8, nq, 0, &ctx));
    OK(lr_context_create(2, M8, nq, 0, &tiny));
    OK(lr_context_create(2 * N, M8, nq, 0, &big));
    lr_poly *a0 = poly(ctx, nq, 2), *a1 = poly(ctx, nq, 2), *a2 = poly(ctx, nq, 2), *b0 = poly(ctx, nq, 2), *b1 = poly(ctx, nq, 2), *o0 = poly(ctx, nq, 2),
            *o1 = poly(ctx, nq, 2), *o2 = poly(ctx, nq, 2);
    lr_poly *narrow = poly(ctx, nq - 1, 2), *single = poly(ctx, nq, 1), *triple = poly(ctx, nq, 3), *wide = poly(big, nq, 2), *s0 = poly(tiny, nq, 2),
            *s1 = poly(tiny, nq, 2), *s2 = poly(tiny, nq, 2), *s3 = poly(tiny, nq, 2);
    lr_poly *inside = nullptr, *alias = nullptr;
    OK(lr_poly_wrap(ctx, device_ptr(o0) + N, nq - 1, 1, &inside));                   // from limb 1 of member 0 of o0 on: a partial overlap
    OK(lr_poly_wrap(ctx, device_ptr(o0), nq, 1, &alias));                            // o0's first member only: the same start, another shape
    const lr_poly *A[2] = {a0, a1}, *B[2] = {b0, b1}, *A3[3] = {a0, a1, a2}, *B3null[3] = {b0, b1, nullptr}, *a_null[2] = {a0, nullptr},
                  *b_null[2] = {nullptr, b1}, *a_out[2] = {a0, o0}, *b_out[2] = {o1, b1}, *a_inside[2] = {inside, a1}, *b_alias[2] = {alias, b1},
                  *a_cross[2] = {o1, o0}, *b_wide[2] = {b0, wide}, *a_narrow[2] = {a0, narrow}, *a_triple[2] = {a0, triple}, *a_single[2] = {a0, single},
                  *T[2] = {s0, s1};
    lr_poly *O[2] = {o0, o1}, *O3[3] = {o0, o1, o2}, *o_null[2] = {o0, nullptr}, *o_same[2] = {o0, o0}, *o_inside[2] = {o0, inside},
            *o_alias[3] = {o0, o1, alias}, *o_narrow[2] = {o0, narrow}, *o_single[2] = {o0, single}, *TO[2] = {s2, s3}, *TO_same[2] = {s2, s2};
    std::vector<uint64_t> w(nq, 1);
    const uint64_t *k = w.data();
    int count = 0;
    // LR_ERR_ARG, in the order of the contract
    REFUSED(lr_ckks_combine(nullptr, LR_ADD, top, 1, A, 1, B, 0, k, k, k, k, k, k, O), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, A, 1, B, 0, k, k, k, k, k, k, nullptr), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, nullptr, 1, B, 0, k, k, k, k, k, k, O), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, 4, top, 1, A, 1, B, 0, k, k, k, k, k, k, O), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, -1, top, 1, A, 1, B, 0, k, k, k, k, k, k, O), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 3, A, 1, B, 0, k, k, k, k, k, k, O), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, -1, A, 1, B, 0, k, k, k, k, k, k, O), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, A, 3, B, 0, k, k, k, k, k, k, O), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, a_null, 1, B, 0, k, k, k, k, k, k, O), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, A, 1, b_null, 0, k, k, k, k, k, k, O), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, A, 2, B3null, 0, k, k, k, k, k, k, O3), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, A, 1, B, 0, k, k, k, k, k, k, o_null), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, A, 1, B, 0, k, nullptr, k, k, k, k, O), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, A, 1, B, 0, k, k, nullptr, k, k, k, O), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, A, 1, B, 0, k, k, k, k, k, nullptr, O), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, A, 1, nullptr, 0, k, k, k, k, k, k, O), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, A, 1, B, 0, k, k, k, k, k, k, o_same), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, A, 1, B, 0, k, k, k, k, k, k, o_inside), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 2, A3, 1, B, 0, k, k, k, k, k, k, o_alias), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, a_out, 1, B, 0, k, k, k, k, k, k, O), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, A, 1, b_out, 0, k, k, k, k, k, k, O), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, a_inside, 1, B, 0, k, k, k, k, k, k, O), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, A, 1, b_alias, 0, k, k, k, k, k, k, O), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, a_cross, 1, B, 0, k, k, k, k, k, k, O), LR_ERR_ARG);
    count += 24;
    // an argument error comes before a shape error, a shape error before the unsupported degree
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top + 5, 1, a_null, 1, B, 0, k, k, k, k, k, k, o_narrow), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(tiny, LR_ADD, top, 1, T, 1, nullptr, 0, k, k, nullptr, nullptr, k, k, TO_same), LR_ERR_ARG);
    REFUSED(lr_ckks_combine(tiny, LR_ADD, top + 1, 1, T, 1, nullptr, 0, k, k, nullptr, nullptr, k, k, TO), LR_ERR_SHAPE);
    count += 3;
    // LR_ERR_SHAPE
    REFUSED(lr_ckks_combine(ctx, LR_ADD, -1, 1, A, 1, B, 0, k, k, k, k, k, k, O), LR_ERR_SHAPE);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, nq, 1, A, 1, B, 0, k, k, k, k, k, k, O), LR_ERR_SHAPE);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, A, 1, b_wide, 0, k, k, k, k, k, k, O), LR_ERR_SHAPE);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, a_narrow, 1, B, 0, k, k, k, k, k, k, O), LR_ERR_SHAPE);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, A, 1, B, 0, k, k, k, k, k, k, o_narrow), LR_ERR_SHAPE);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, A, 1, B, 0, k, k, k, k, k, k, o_single), LR_ERR_SHAPE);
    REFUSED(lr_ckks_combine(ctx, LR_ADD, top, 1, a_triple, 1, B, 0, k, k, k, k, k, k, O), LR_ERR_SHAPE);
    {   // component and batch member share grid z
        lr_poly *m0 = poly(ctx, 1, 32768), *m1 = poly(ctx, 1, 32768);
        const lr_poly *many[1] = {m0};
        lr_poly *many_out[1] = {m1};
        REFUSED(lr_ckks_combine(ctx, LR_ADD, 0, 0, many, 0, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, many_out), LR_ERR_SHAPE);
        for (lr_poly *p : {m0, m1}) lr_poly_free(p);
        lr_poly *t0 = poly(ctx, 1, 21846), *t1 = poly(ctx, 1, 21846), *t2 = poly(ctx, 1, 21846);
        const lr_poly *three[3] = {single, single, single};
        lr_poly *three_out[3] = {t0, t1, t2};
        REFUSED(lr_ckks_combine(ctx, LR_ADD, 0, 2, three, 0, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, three_out), LR_ERR_SHAPE);
        for (lr_poly *p : {t0, t1, t2}) lr_poly_free(p);
    }
    count += 9;
    OK(lr_ckks_combine(ctx, LR_ADD, top - 1, 1, a_narrow, 1, B, 0, k, k, k, k, k, k, O));                       // ... which is enough one level down
    OK(lr_ckks_combine(ctx, LR_ADD, top, 1, a_single, 1, B, 0, k, k, k, k, k, k, O));                           // an operand of batch 1 is read by every member
    // LR_ERR_UNSUPPORTED
    REFUSED(lr_ckks_combine(tiny, LR_ADD, top, 1, T, 1, nullptr, 0, k, k, nullptr, nullptr, k, k, TO), LR_ERR_UNSUPPORTED);
    count += 1;
    // the constants function: one refusal per message (the word-for-word domain is the oracle test's business)
    {
        const uint64_t even[3] = {M8[0] + 1, M8[1], M8[2]};
        int la = -7, da = -7, ms = -7;
        double sa = -7;
        uint64_t o[3] = {7, 7, 7};
        const double D = 1099511627776.0;
        REFUSED(lr_ckks_combine_constants(nullptr, 3, LR_ADD, 1, 2, D, 1, 2, D, 1, 2, D, 0, &la, &sa, &da, &ms, o), LR_ERR_ARG);
        REFUSED(lr_ckks_combine_constants(M8, 3, LR_ADD, 1, 3, D, 1, 2, D, 1, 2, D, 0, &la, &sa, &da, &ms, o), LR_ERR_ARG);
        REFUSED(lr_ckks_combine_constants(even, 3, LR_ADD, 1, 2, D, 1, 2, D, 1, 2, D, 0, &la, &sa, &da, &ms, o), LR_ERR_ARG);
        REFUSED(lr_ckks_combine_constants(M8, 3, LR_ADD, 1, 2, -D, 1, 2, D, 1, 2, D, 0, &la, &sa, &da, &ms, o), LR_ERR_ARG);
        REFUSED(lr_ckks_combine_constants(M8, 3, LR_ADD, 1, 2, D, 1, 2, D, 1, 1, D, LR_COMBINE_OUT_A, &la, &sa, &da, &ms, o), LR_ERR_ARG);
        REFUSED(lr_ckks_combine_constants(M8, 3, LR_ADD, 1, 2, 1.0, 1, 2, 1e19, 1, 2, D, 0, &la, &sa, &da, &ms, o), LR_ERR_ARG);
        REFUSED(lr_ckks_combine_constants(M8, 3, LR_SUB, 0, 2, D, 0, 2, D, 1, 2, D, 0, &la, &sa, &da, &ms, o), LR_ERR_UNSUPPORTED);
        REFUSED(lr_ckks_combine_constants(M8, 3, LR_SUB, 2, 2, D, 1, 2, D, 1, 2, D, 0, &la, &sa, &da, &ms, o), LR_ERR_UNSUPPORTED);
        REFUSED(lr_ckks_combine_constants(M8, 3, LR_SUB, 1, 2, D, 1, 2, D, 1, 1, D, 0, &la, &sa, &da, &ms, o), LR_ERR_UNSUPPORTED);
        REFUSED(lr_ckks_combine_constants(M8, 3, LR_SUB, 2, 2, D, 1, 2, 2 * D, 2, 2, D, 0, &la, &sa, &da, &ms, o), LR_ERR_UNSUPPORTED);
        CHECK(la == -7 && da == -7 && ms == -7 && sa == -7 && o[0] == 7 && o[1] == 7 && o[2] == 7);
        count += 10;
    }
    for (lr_poly *p : {a0, a1, a2, b0, b1, o0, o1, o2, narrow, single, triple, wide, s0, s1, s2, s3, inside, alias}) lr_poly_free(p);
    OK(lr_context_destroy(big));
    OK(lr_context_destroy(tiny));
    OK(lr_context_destroy(ctx));
    return count;
}

// lr_ckks_combine_constants holds no state: two threads run the same call over and over and must read the same words, and each reads
// its own refusal text
static void constants_worker(int id, std::atomic<int> *done) {
    const double D = 1099511627776.0;
    std::vector<uint64_t> first;
    for (int round = 0; round < 200; ++round) {
        int la = 0, da = 0, ms = 0;
        double sa = 0;
        std::vector<uint64_t> words(8);
        OK(lr_ckks_combine_constants(M8, 8, LR_SUB, 1, 6, D * 1.5, 2, 5, D * 1048577.75, 2, 7, D, LR_COMBINE_OUT_NEW, &la, &sa, &da, &ms, words.data()));
        CHECK(la == 5 && da == 2 && ms == 1 && sa == D * 1048577.75);
        words.resize(6);
        if (round == 0) first = words;
        CHECK(words == first);
        const int rc = id ? lr_ckks_combine_constants(M8, 8, LR_SUB, 1, 7, -1.0, 1, 7, D, 1, 7, D, 0, &la, &sa, &da, &ms, words.data())
                          : lr_ckks_combine_constants(M8, 8, LR_SUB, 0, 7, D, 0, 7, D, 1, 7, D, 0, &la, &sa, &da, &ms, words.data());
        CHECK(rc == (id ? LR_ERR_ARG : LR_ERR_UNSUPPORTED));
        CHECK(std::string(lr_last_error_string()).find(id ? "a scale is not finite" : "both operands have degree 0") != std::string::npos);
    }
    done->fetch_add(1);
}

int main() {
    int calls = 0;
    {
        const uint64_t N = 16;
        const int nq = 8;
        lr_context *ctx = nullptr;
        OK(lr_context_create(N, M8, nq, 0, &ctx));
        // every degree pair x every flag combination; the operation, the level, the batch, the view and the shared operand cycle
        for (int deg_a = 0; deg_a <= 2; ++deg_a)
            for (int deg_b = -1; deg_b <= 2; ++deg_b)
                for (unsigned flags = 0; flags < 16; ++flags) {
                    const int n = calls;
                    const int batch = n % 3 == 0 ? 1 : 3, shared = batch == 1 ? 0 : (n % 5 == 1 ? 1 : n % 5 == 2 && deg_b >= 0 ? 2 : 0);
                    one_call(ctx, N, nq, n % 4 == 0 ? nq - 1 : n % 7, n % 4, deg_a, deg_b, flags, batch, 0, shared, n % 2 == 1);
                    ++calls;
                }
        // the receiver is a, b, both
        for (int op = 0; op < 4; ++op) {
            one_call(ctx, N, nq, 4, op, 1, 1, 6u, 3, 1, 0, false);
            one_call(ctx, N, nq, 4, op, 2, 1, 3u, 2, 1, 2, true);
            one_call(ctx, N, nq, 7, op, 1, 2, 15u, 1, 1, 0, false);       // out_2 is a fresh poly
            one_call(ctx, N, nq, 4, op, 1, 2, 12u, 3, 2, 1, true);
            one_call(ctx, N, nq, 0, op, 0, 1, 4u, 2, 2, 0, false);
            one_call(ctx, N, nq, 5, op, 1, 1, 1u, 3, 3, 0, true);
            one_call(ctx, N, nq, 7, op, 2, 2, 9u, 1, 3, 0, false);
            calls += 7;
        }
        OK(lr_context_destroy(ctx));
    }
    {   // N = 2^12, the smallest degree with more than one workgroup per row
        lr_context *ctx = nullptr;
        OK(lr_context_create(1 << 12, M8, 3, 0, &ctx));
        one_call(ctx, 1 << 12, 3, 2, LR_SUB, 1, 2, 15u, 2, 1, 0, true);
        ++calls;
        OK(lr_context_destroy(ctx));
    }
    const int refused = refusals();
    {
        std::atomic<int> done{0};
        std::thread a(constants_worker, 0, &done), b(constants_worker, 1, &done);
        a.join();
        b.join();
        CHECK(done.load() == 2);
    }
    return driver_end(ALLOCATIONS | EVENTS | LOG, refused, "ckks combine: calls %d, launches %llu, refusals %d", calls, lr::g_combine_launches.load(), refused);
}
