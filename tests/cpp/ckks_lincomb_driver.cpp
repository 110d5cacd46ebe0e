// The host side of the CKKS linear combination under AddressSanitizer + UBSan and under ThreadSanitizer
// (tests/test_host_ckks_lincomb_sanitizers.py): the REAL host code -- lr_abi_*.cpp (lr_abi_ckks_eval.cpp, lr_abi_ckks_scalar.cpp), lr_host.hpp,
// lr_precompute.cpp -- compiled with g++ against the host-only HIP stand-in and the recording launch stubs of tests/cpp/hipstub/; the
// stand-in of the pass's launcher keeps every launch and touches the first and the last word of every row a kernel would read or write.  Every refusal in the stated order with the message its caller reads; the split of 0, 1, 16, 17 and 33
// terms into launches -- the term ranges, the accumulate flags, the constant on the first pass only, the limb ranges and the words of
// every limb -- on polys whose members lie apart by more than their limbs and at a level below their limb count; the constants function
// on two threads.  Exit code 0 = every check held; a sanitizer report aborts the run.  Nothing here computes on polys: parity is the GPU
// suite's business.
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
struct LinCombRecord {
    LinCombLaunch L;
    int limbs, batch;
};
extern std::atomic<unsigned long long> g_stub_launches, g_lincomb_launches;
extern std::mutex g_lincomb_mu;
extern std::vector<LinCombRecord> g_lincomb_log;
}  // namespace lr

#define REFUSED REFUSED_MSG_NO_LAUNCH      // here a refusal launches nothing of any kind and is logged with its message
#include "driver_check.hpp"

static std::vector<lr::LinCombRecord> take_log() {
    std::lock_guard<std::mutex> lock(lr::g_lincomb_mu);
    std::vector<lr::LinCombRecord> out;
    out.swap(lr::g_lincomb_log);
    return out;
}

static uint64_t *device_ptr(const lr_poly *p) {
    uint64_t *d = nullptr;
    OK(lr_poly_info(p, nullptr, nullptr, nullptr, (void **)&d));
    return d;
}

// the launches of one accepted call against what the contract says they carry; returns their number
static int splits(lr_context *ctx, uint64_t N, int nq, int level, int T, int batch, bool with_const, bool accumulate, bool strided) {
    const int L1 = level + 1;
    // terms and receiver with one limb more than the level needs; strided: members two limbs further apart (a view into a larger poly)
    const int limbs = L1 + (level + 1 < nq ? 1 : 0);
    const long long stride = (long long)(limbs + (strided ? 2 : 0)) * (long long)N;
    std::vector<void *> raw;
    const auto make = [&]() -> lr_poly * {
        if (!strided) return poly(ctx, limbs, batch);
        void *d = nullptr;
        CHECK(hipMalloc(&d, (size_t)((batch - 1) * stride + (long long)limbs * (long long)N) * sizeof(uint64_t)) == hipSuccess);   // exactly what the view spans
        raw.push_back(d);
        lr_poly *p = nullptr;
        OK(lr_poly_wrap_strided(ctx, d, limbs, batch, stride, &p));
        return p;
    };
    std::vector<lr_poly *> own;
    std::vector<const lr_poly *> t0, t1;
    for (int k = 0; k < T; ++k) {
        if (k == 3) {     // a term listed twice
            t0.push_back(t0[1]);
            t1.push_back(t1[1]);
            continue;
        }
        own.push_back(make());
        t0.push_back(own.back());
        own.push_back(make());
        t1.push_back(own.back());
    }
    lr_poly *o0 = make(), *o1 = make();
    // exactly [T] and [T][level + 1] words, every one distinct
    std::vector<uint8_t> has_pre((size_t)T);
    std::vector<uint64_t> pre((size_t)T * L1), lo((size_t)T * L1), hi((size_t)T * L1), add_lo((size_t)L1), add_hi((size_t)L1);
    for (int k = 0; k < T; ++k) {
        has_pre[k] = (uint8_t)(k % 3 == 1);
        for (int i = 0; i < L1; ++i) {
            const uint64_t id = (uint64_t)k * 100 + (uint64_t)i;
            pre[(size_t)k * L1 + i] = 1000000 + id;
            lo[(size_t)k * L1 + i] = 2000000 + id;
            hi[(size_t)k * L1 + i] = 3000000 + id;
        }
    }
    for (int i = 0; i < L1; ++i) {
        add_lo[i] = 4000000 + (uint64_t)i;
        add_hi[i] = 5000000 + (uint64_t)i;
    }
    (void)take_log();
    OK(lr_ckks_lincomb(ctx, level, T, t0.data(), t1.data(), has_pre.data(), pre.data(), lo.data(), hi.data(), with_const ? add_lo.data() : nullptr,
                       with_const ? add_hi.data() : nullptr, accumulate ? 1 : 0, o0, o1));
    const std::vector<lr::LinCombRecord> log = take_log();
    // walk the launches in order: passes of at most 16 terms, within a pass the limb ranges from 0 up
    size_t at = 0;
    int first = 0;
    const bool nothing = T == 0 && !with_const && accumulate;
    if (nothing) CHECK(log.empty());
    while (!nothing) {
        const int count = std::min(T - first, lr::kLinCombTerms);
        const int has_add = first == 0 && with_const ? 1 : 0;
        const int words = lr::lincomb_limb_words(count, has_add), step = lr::lincomb_limbs_per_launch(count, has_add);
        for (int limb0 = 0; limb0 < L1; limb0 += step, ++at) {
            CHECK(at < log.size());
            if (at >= log.size()) break;
            const lr::LinCombRecord &r = log[at];
            const lr::LinCombLaunch &L = r.L;
            CHECK(r.batch == batch && r.limbs == std::min(step, L1 - limb0) && L.limb0 == limb0 && L.n == (int)N);
            CHECK(L.count == count && L.has_add == has_add && L.accumulate == ((first > 0 || accumulate) ? 1 : 0));
            CHECK(L.out[0] == device_ptr(o0) && L.out[1] == device_ptr(o1) && L.out_stride[0] == stride && L.out_stride[1] == stride);
            unsigned mask = 0;
            for (int k = 0; k < count; ++k) {
                CHECK(L.term[k].c[0] == device_ptr(t0[first + k]) && L.term[k].c[1] == device_ptr(t1[first + k]));
                CHECK(L.term[k].stride[0] == stride && L.term[k].stride[1] == stride);
                if (has_pre[first + k]) mask |= 1u << k;
            }
            CHECK(L.pre_mask == mask);
            for (int y = 0; y < r.limbs; ++y) {
                const uint64_t *w = L.k + (size_t)y * words;
                const int i = limb0 + y;
                if (has_add) {
                    CHECK(w[0] == add_lo[i] && w[1] == add_hi[i]);
                    w += 2;
                }
                for (int k = 0; k < count; ++k) {
                    const size_t src = (size_t)(first + k) * L1 + i;
                    CHECK(w[3 * k] == (has_pre[first + k] ? pre[src] : 0) && w[3 * k + 1] == lo[src] && w[3 * k + 2] == hi[src]);
                }
            }
        }
        first += count;
        if (first >= T) break;
    }
    CHECK(at == log.size());
    const int passes = T == 0 ? (nothing ? 0 : 1) : (T + lr::kLinCombTerms - 1) / lr::kLinCombTerms;
    std::printf("split T=%2d level=%d batch=%d const=%d accumulate=%d strided=%d: %d passes, %zu launches\n", T, level, batch, (int)with_const,
                (int)accumulate, (int)strided, passes, log.size());
    OK(lr_context_sync(ctx));
    for (lr_poly *p : own) lr_poly_free(p);
    lr_poly_free(o0);
    lr_poly_free(o1);
    for (void *d : raw) (void)hipFree(d);
    return (int)log.size();
}

static int refusals() {
    const uint64_t N = 16;
    const int nq = 3, top = 2;
    lr_context *ctx = nullptr, *tiny = nullptr, *big = nullptr;
    OK(lr_context_create(N, M8, nq, 0, &ctx));
    OK(lr_context_create(2, M8, nq, 0, &tiny));
    OK(lr_context_create(2 * N, M8, nq, 0, &big));
    lr_poly *a0 = poly(ctx, nq, 2), *a1 = poly(ctx, nq, 2), *b0 = poly(ctx, nq, 2), *b1 = poly(ctx, nq, 2), *o0 = poly(ctx, nq, 2), *o1 = poly(ctx, nq, 2);
    lr_poly *narrow = poly(ctx, nq - 1, 2), *single = poly(ctx, nq, 1), *wide = poly(big, nq, 2), *s0 = poly(tiny, nq, 2), *s1 = poly(tiny, nq, 2),
            *s2 = poly(tiny, nq, 2), *s3 = poly(tiny, nq, 2);
    lr_poly *inside = nullptr;                                                       // from limb 1 of member 0 of o0 on: a partial overlap
    OK(lr_poly_wrap(ctx, device_ptr(o0) + N, nq - 1, 1, &inside));
    const lr_poly *t0[2] = {a0, b0}, *t1[2] = {a1, b1}, *with_null[2] = {a0, nullptr}, *with_out[2] = {a0, o1}, *with_narrow[2] = {a0, narrow},
                  *with_single[2] = {single, b0}, *with_wide[2] = {a0, wide}, *tiny0[1] = {s0}, *tiny1[1] = {s1}, *with_inside[2] = {a0, inside};
    const uint8_t hp[2] = {0, 1};
    std::vector<uint64_t> w(2 * nq, 1);
    const uint64_t *k = w.data();
    int count = 0;
    // LR_ERR_ARG, in the order of the contract
    REFUSED(lr_ckks_lincomb(nullptr, top, 2, t0, t1, hp, k, k, k, k, k, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, t0, t1, hp, k, k, k, k, k, 0, nullptr, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, t0, t1, hp, k, k, k, k, k, 0, o0, nullptr), LR_ERR_ARG);
    REFUSED(lr_ckks_lincomb(ctx, top, -1, t0, t1, hp, k, k, k, k, k, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, nullptr, t1, hp, k, k, k, k, k, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, t0, nullptr, hp, k, k, k, k, k, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, t0, t1, nullptr, k, k, k, k, k, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, t0, t1, hp, nullptr, k, k, k, k, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, t0, t1, hp, k, nullptr, k, k, k, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, t0, t1, hp, k, k, nullptr, k, k, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, with_null, t1, hp, k, k, k, k, k, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, t0, with_null, hp, k, k, k, k, k, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, t0, t1, hp, k, k, k, k, nullptr, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, t0, t1, hp, k, k, k, nullptr, k, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, t0, t1, hp, k, k, k, k, k, 0, o0, o0), LR_ERR_ARG);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, t0, t1, hp, k, k, k, k, k, 0, o0, inside), LR_ERR_ARG);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, t0, with_out, hp, k, k, k, k, k, 1, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, with_inside, t1, hp, k, k, k, k, k, 0, o0, o1), LR_ERR_ARG);
    count += 18;
    // an argument error comes before a shape error, a shape error before the unsupported degree
    REFUSED(lr_ckks_lincomb(ctx, top + 5, 2, with_null, with_narrow, hp, k, k, k, k, k, 0, o0, o1), LR_ERR_ARG);
    REFUSED(lr_ckks_lincomb(tiny, top, 1, tiny0, tiny1, hp, k, k, k, k, k, 0, s2, s2), LR_ERR_ARG);
    REFUSED(lr_ckks_lincomb(tiny, top + 1, 1, tiny0, tiny1, hp, k, k, k, k, k, 0, s2, s3), LR_ERR_SHAPE);
    count += 3;
    // LR_ERR_SHAPE
    REFUSED(lr_ckks_lincomb(ctx, -1, 2, t0, t1, hp, k, k, k, k, k, 0, o0, o1), LR_ERR_SHAPE);
    REFUSED(lr_ckks_lincomb(ctx, nq, 2, t0, t1, hp, k, k, k, k, k, 0, o0, o1), LR_ERR_SHAPE);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, t0, with_wide, hp, k, k, k, k, k, 0, o0, o1), LR_ERR_SHAPE);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, t0, with_narrow, hp, k, k, k, k, k, 0, o0, o1), LR_ERR_SHAPE);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, t0, t1, hp, k, k, k, k, k, 0, o0, narrow), LR_ERR_SHAPE);
    REFUSED(lr_ckks_lincomb(ctx, top, 2, with_single, t1, hp, k, k, k, k, k, 0, o0, o1), LR_ERR_SHAPE);      // no broadcast: every poly the same batch
    REFUSED(lr_ckks_lincomb(ctx, top, 2, t0, t1, hp, k, k, k, k, k, 0, single, o1), LR_ERR_SHAPE);
    {   // component and batch member share grid z
        lr_poly *m0 = poly(ctx, 1, 32768), *m1 = poly(ctx, 1, 32768), *m2 = poly(ctx, 1, 32768), *m3 = poly(ctx, 1, 32768);
        const lr_poly *many0[1] = {m0}, *many1[1] = {m1};
        REFUSED(lr_ckks_lincomb(ctx, 0, 1, many0, many1, hp, k, k, k, k, k, 0, m2, m3), LR_ERR_SHAPE);
        for (lr_poly *p : {m0, m1, m2, m3}) lr_poly_free(p);
    }
    count += 8;
    OK(lr_ckks_lincomb(ctx, top - 1, 2, t0, with_narrow, hp, k, k, k, k, k, 0, o0, o1));                      // ... which is enough one level down
    // LR_ERR_UNSUPPORTED
    REFUSED(lr_ckks_lincomb(tiny, top, 1, tiny0, tiny1, hp, k, k, k, k, k, 0, s2, s3), LR_ERR_UNSUPPORTED);
    REFUSED(lr_ckks_lincomb(tiny, top, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, k, k, 0, s2, s3), LR_ERR_UNSUPPORTED);
    count += 2;
    // the constants function: one refusal per message (the word-for-word domain is the oracle test's business)
    {
        const uint64_t psi[3] = {5, 5, 5}, even[3] = {M8[0] + 1, M8[1], M8[2]};
        const double re[1] = {0.5}, im[1] = {0}, sc[1] = {1099511627776.0}, huge[1] = {4e18}, big_scale[1] = {1e300}, tiny_scale[1] = {1e-300};
        const int lv[1] = {2}, bad_lv[1] = {3};
        int la = -7;
        double sa = -7;
        uint64_t o[3] = {7, 7, 7};
        uint8_t h[1] = {7};
        const double D = 1099511627776.0;
        REFUSED(lr_ckks_lincomb_constants(nullptr, psi, 3, D, 2, D, 0, 0, 0, 1, re, im, sc, lv, &la, &sa, o, o, h, o, o, o), LR_ERR_ARG);
        REFUSED(lr_ckks_lincomb_constants(M8, psi, 3, D, 2, D, 0, 0, 0, 1, re, im, sc, bad_lv, &la, &sa, o, o, h, o, o, o), LR_ERR_ARG);
        REFUSED(lr_ckks_lincomb_constants(even, psi, 3, D, 2, D, 0, 0, 0, 1, re, im, sc, lv, &la, &sa, o, o, h, o, o, o), LR_ERR_ARG);
        REFUSED(lr_ckks_lincomb_constants(M8, M8, 3, D, 2, D, 0, 0, 0, 1, re, im, sc, lv, &la, &sa, o, o, h, o, o, o), LR_ERR_ARG);
        REFUSED(lr_ckks_lincomb_constants(M8, psi, 3, D, 2, -D, 0, 0, 0, 1, re, im, sc, lv, &la, &sa, o, o, h, o, o, o), LR_ERR_ARG);
        REFUSED(lr_ckks_lincomb_constants(M8, psi, 3, D, 2, D, 1, 1e19, 0, 1, re, im, sc, lv, &la, &sa, o, o, h, o, o, o), LR_ERR_ARG);
        REFUSED(lr_ckks_lincomb_constants(M8, psi, 3, D, 2, 1.0, 0, 0, 0, 1, huge, im, big_scale, lv, &la, &sa, o, o, h, o, o, o), LR_ERR_ARG);
        REFUSED(lr_ckks_lincomb_constants(M8, psi, 3, D, 2, 1e300, 0, 0, 0, 1, huge, im, tiny_scale, lv, &la, &sa, o, o, h, o, o, o), LR_ERR_ARG);
        CHECK(la == -7 && sa == -7 && o[0] == 7 && o[1] == 7 && o[2] == 7 && h[0] == 7);
        count += 8;
    }
    for (lr_poly *p : {a0, a1, b0, b1, o0, o1, narrow, single, wide, s0, s1, s2, s3, inside}) lr_poly_free(p);
    OK(lr_context_destroy(big));
    OK(lr_context_destroy(tiny));
    OK(lr_context_destroy(ctx));
    return count;
}

// lr_ckks_lincomb_constants holds no state: two threads run the same chain over and over and must read the same words, and each reads
// its own refusal text
static void constants_worker(int id, std::atomic<int> *done) {
    const uint64_t psi[8] = {3, 5, 7, 9, 11, 13, 15, 17};
    const double D = 1099511627776.0;
    const double re[4] = {0.5, -3, 0.25, 7}, im[4] = {-0.125, 0, 0.75, -2}, sc[4] = {D, D * 1.5, D * (1 + 1.0 / 1048576), D / 4};
    const int lv[4] = {7, 5, 6, 7};
    std::vector<uint64_t> first;
    for (int round = 0; round < 200; ++round) {
        int la = 0;
        double sa = 0;
        std::vector<uint64_t> add_lo(8), add_hi(8), words(3 * 4 * 8);
        uint8_t hp[4];
        OK(lr_ckks_lincomb_constants(M8, psi, 8, D, 7, D, 1, 0.3, -0.4, 4, re, im, sc, lv, &la, &sa, add_lo.data(), add_hi.data(), hp, words.data(),
                                     words.data() + 32, words.data() + 64));
        CHECK(la == 5 && std::isfinite(sa));
        words.insert(words.end(), add_lo.begin(), add_lo.end());
        words.insert(words.end(), hp, hp + 4);
        if (round == 0) first = words;
        CHECK(words == first);
        const int rc = id ? lr_ckks_lincomb_constants(M8, psi, 8, -1.0, 7, D, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, &la, &sa, nullptr, nullptr,
                                                      nullptr, nullptr, nullptr, nullptr)
                          : lr_ckks_lincomb_constants(M8, psi, 8, D, 9, D, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, &la, &sa, nullptr, nullptr,
                                                      nullptr, nullptr, nullptr, nullptr);
        CHECK(rc == LR_ERR_ARG);
        CHECK(std::string(lr_last_error_string()).find(id ? "a scale is not finite" : "a level is out of range") != std::string::npos);
    }
    done->fetch_add(1);
}

int main() {
    int launches = 0, calls = 0;
    {
        const uint64_t N = 16;
        const int nq = 8;
        lr_context *ctx = nullptr;
        OK(lr_context_create(N, M8, nq, 0, &ctx));
        for (int T : {0, 1, 16, 17, 33})
            for (int variant = 0; variant < 4; ++variant) {
                const bool with_const = variant != 1, accumulate = variant >= 2, strided = variant == 3;
                const int level = variant == 2 ? 4 : nq - 1, batch = variant == 0 ? 1 : 3;
                launches += splits(ctx, N, nq, level, T, batch, with_const, accumulate, strided);
                ++calls;
            }
        launches += splits(ctx, N, nq, 2, 0, 2, false, true, false);      // nothing to do: no launch
        ++calls;
        OK(lr_context_destroy(ctx));
    }
    {   // N = 2^12, the smallest degree with more than one workgroup per row
        lr_context *ctx = nullptr;
        OK(lr_context_create(1 << 12, M8, 3, 0, &ctx));
        launches += splits(ctx, 1 << 12, 3, 2, 17, 2, true, false, true);
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
    return driver_end(ALLOCATIONS | EVENTS | LOG, refused, "ckks lincomb: calls %d, launches %d, refusals %d", calls, launches, refused);
}
