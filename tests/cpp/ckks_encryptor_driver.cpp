// The CKKS encryptor's host side under AddressSanitizer + UBSan and under ThreadSanitizer (tests/test_host_ckks_encryptor_sanitizers.py):
// the REAL host code -- lr_ckks_encryptor.cpp with every other host unit of the library -- compiled with g++ against the host-only HIP
// stand-in and the launch stand-ins of tests/cpp/hipstub/, which touch the first and the last byte of everything a kernel would read or
// write.  pk and sk, fast and through P, the top level and level 0, host and device-pointer randomness, both shapes
// (lr_options::no_epilogue), batches 1, 3 and max_batch with the pools and the staging buffer reused across consecutive host-form calls,
// wide polys, shared and per-ciphertext keys; two handles on two threads; the launch counts of the fast forms; every refusal.
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
extern std::atomic<unsigned long long> g_stub_launches, g_encryptor_stub_launches, g_ckks_expand_launches, g_ckks_fast_launches;
}  // namespace lr

static const int NQ = 3, NP = 1, MAXB = 5;

static unsigned long long launches() { return lr::g_stub_launches.load() + lr::g_encryptor_stub_launches.load(); }

// one encryptor through every call shape; returns the number of accepted calls
static int exercise(uint64_t N, const lr_options *opt) {
    Rings r(N, Qm, NQ, NP, opt);
    lr_ckks_encryptor *enc = nullptr;
    OK(opt ? lr_ckks_encryptor_create_ex(r.q, r.p, MAXB, opt, &enc) : lr_ckks_encryptor_create(r.q, r.p, MAXB, &enc));
    if (!enc) return 0;
    int calls = 0;
    for (int round = 0; round < 2; ++round)                                   // the second round reuses the pools and the staging buffer
        for (int batch : {1, 3, MAXB}) {
            const bool wide = (batch + round) % 2 == 1;                       // polys with one limb more than needed: another stride
            const int kb = round == 0 ? 1 : batch;                            // keys and plaintext: one for the batch, or one each
            lr_poly *pk0 = poly(r.q, NQ + NP + (wide ? 1 : 0), kb), *pk1 = poly(r.q, NQ + NP, kb), *sk = poly(r.q, NQ + NP, kb);
            lr_poly *crp = poly(r.q, NQ + NP + (wide ? 0 : 1), batch);
            // exactly [batch][N / 8] and [batch][N] bytes
            std::vector<uint8_t> uc((size_t)batch * N / 8, 0xAA), us((size_t)batch * N / 8, 0xCC), e0((size_t)batch * N, 0x93), e1((size_t)batch * N, 0);
            void *duc = nullptr, *dus = nullptr, *de0 = nullptr, *de1 = nullptr;
            CHECK(hipMalloc(&duc, uc.size()) == hipSuccess && hipMalloc(&dus, us.size()) == hipSuccess);
            CHECK(hipMalloc(&de0, e0.size()) == hipSuccess && hipMalloc(&de1, e1.size()) == hipSuccess);
            for (int level : {NQ - 1, 0}) {
                // plaintext and ciphertext with exactly level + 1 limbs (or one more): a limb above the level touched is a report
                lr_poly *pt = poly(r.q, level + 1, kb), *c0 = poly(r.q, wide ? level + 2 : level + 1, batch), *c1 = poly(r.q, level + 1, batch);
                for (int fast : {0, 1}) {
                    const unsigned long long before = launches();
                    // two host-form calls one behind the other: the second refills the pinned buffer the first one staged through
                    OK(lr_ckks_encryptor_encrypt_pk(enc, fast, level, pk0, pk1, uc.data(), us.data(), e0.data(), e1.data(), pt, batch, c0, c1));
                    OK(lr_ckks_encryptor_encrypt_sk(enc, fast, level, sk, crp, e0.data(), pt, batch, c0, c1));
                    OK(lr_ckks_encryptor_encrypt_pk_device(enc, fast, level, pk0, pk1, duc, dus, de0, de1, pt, batch, c0, c1));
                    OK(lr_ckks_encryptor_encrypt_sk_device(enc, fast, level, sk, crp, de1, pt, batch, c0, c1));
                    CHECK(launches() - before >= 4 * 3);
                    calls += 4;
                }
                for (lr_poly *p : {pt, c0, c1}) lr_poly_free(p);
            }
            OK(lr_context_sync(r.q));
            for (void *p : {duc, dus, de0, de1}) (void)hipFree(p);
            for (lr_poly *p : {pk0, pk1, sk, crp}) lr_poly_free(p);
        }
    OK(lr_ckks_encryptor_destroy(enc));
    return calls;
}

// the fast forms at N = 2^4, where a transform is one launch: the default shape is expansion, ONE transform, ONE pass
static void sequences() {
    const uint64_t N = 16;
    const int batch = 2, level = NQ - 1;
    for (int call_by_call : {0, 1}) {
        lr_options opt;
        OK(lr_options_init(&opt));
        opt.no_epilogue = call_by_call;
        Rings r(N, Qm, NQ, NP, &opt);
        lr_ckks_encryptor *enc = nullptr;
        OK(lr_ckks_encryptor_create_ex(r.q, nullptr, batch, &opt, &enc));           // P empty: the fast forms need no extender
        lr_poly *pk0 = poly(r.q, NQ, 1), *pk1 = poly(r.q, NQ, 1), *crp = poly(r.q, NQ, batch), *pt = poly(r.q, NQ, 1), *c0 = poly(r.q, NQ, batch),
                *c1 = poly(r.q, NQ, batch);
        std::vector<uint8_t> bits((size_t)batch * N / 8, 0xFF), noise((size_t)batch * N, 0x80);
        unsigned long long s0 = lr::g_stub_launches.load(), x0 = lr::g_ckks_expand_launches.load(), f0 = lr::g_ckks_fast_launches.load();
        OK(lr_ckks_encryptor_encrypt_pk(enc, 1, level, pk0, pk1, bits.data(), bits.data(), noise.data(), noise.data(), pt, batch, c0, c1));
        if (call_by_call) {
            // ckks/encryptor.go:187-200, :234: SampleTernaryMontgomeryNTT, two MulCoeffsMontgomery, SampleNTT + Add twice, the Add of the plaintext
            CHECK(lr::g_ckks_expand_launches.load() - x0 == 3 && lr::g_ckks_fast_launches.load() - f0 == 0);
            CHECK(lr::g_stub_launches.load() - s0 == 1 + 2 + 2 * 2 + 1);
        } else {
            CHECK(lr::g_ckks_expand_launches.load() - x0 == 1 && lr::g_ckks_fast_launches.load() - f0 == 1);
            CHECK(lr::g_stub_launches.load() - s0 == 1);
        }
        s0 = lr::g_stub_launches.load(), x0 = lr::g_ckks_expand_launches.load(), f0 = lr::g_ckks_fast_launches.load();
        OK(lr_ckks_encryptor_encrypt_sk(enc, 1, level, pk0, crp, noise.data(), pt, batch, c0, c1));
        if (call_by_call) {
            // :324-330, :359: SampleNTT, MulCoeffsMontgomery, Neg, Add, Copy, the Add of the plaintext
            CHECK(lr::g_ckks_expand_launches.load() - x0 == 1 && lr::g_ckks_fast_launches.load() - f0 == 0);
            CHECK(lr::g_stub_launches.load() - s0 == 1 + 5);
        } else {
            CHECK(lr::g_ckks_expand_launches.load() - x0 == 1 && lr::g_ckks_fast_launches.load() - f0 == 1);
            CHECK(lr::g_stub_launches.load() - s0 == 1);
        }
        for (lr_poly *p : {pk0, pk1, crp, pt, c0, c1}) lr_poly_free(p);
        OK(lr_ckks_encryptor_destroy(enc));
    }
}

static int refusals() {
    const uint64_t N = 16;
    const int top = NQ - 1;
    int count = 0;
    Rings r(N, Qm, NQ, NP, nullptr), other(N, Qm, NQ, NP, nullptr);
    lr_context *small = nullptr, *big = nullptr;
    OK(lr_context_create(4, Qm, NQ, 0, &small));
    OK(lr_context_create(2 * N, Qm + NQ, NP, 0, &big));
    lr_context *dev1 = nullptr;
    OK(lr_context_create(N, Qm + NQ, NP, 1, &dev1));
    lr_ckks_encryptor *enc = nullptr, *none = nullptr, *fast_only = nullptr;
    const unsigned long long before = launches();
    // creation
    REFUSED(lr_ckks_encryptor_create(nullptr, r.p, 1, &none) == LR_ERR_ARG);
    REFUSED(lr_ckks_encryptor_create(r.q, r.p, 1, nullptr) == LR_ERR_ARG);
    REFUSED(lr_ckks_encryptor_create(r.q, r.p, 0, &none) == LR_ERR_ARG && none == nullptr);
    REFUSED(lr_ckks_encryptor_create(r.q, r.p, 65536, &none) == LR_ERR_ARG);
    REFUSED(lr_ckks_encryptor_create(small, nullptr, 1, &none) == LR_ERR_ARG);                 // N < 8
    REFUSED(lr_ckks_encryptor_create(r.q, big, 1, &none) == LR_ERR_ARG);                       // ctxP with another N
    REFUSED(lr_ckks_encryptor_create(r.q, dev1, 1, &none) == LR_ERR_ARG);                      // ctxP on another device
    lr_options bad;
    OK(lr_options_init(&bad));
    bad.version = 99;
    REFUSED(lr_ckks_encryptor_create_ex(r.q, r.p, 1, &bad, &none) == LR_ERR_ARG);
    count += 8;
    OK(lr_ckks_encryptor_create(r.q, r.p, 2, &enc));
    OK(lr_ckks_encryptor_create(r.q, nullptr, 2, &fast_only));
    lr_poly *pk0 = poly(r.q, NQ + NP, 1), *pk1 = poly(r.q, NQ + NP, 1), *sk = poly(r.q, NQ + NP, 1), *crp = poly(r.q, NQ + NP, 2), *pt = poly(r.q, NQ, 2);
    lr_poly *c0 = poly(r.q, NQ, 2), *c1 = poly(r.q, NQ, 2), *foreign = poly(other.q, NQ + NP, 2), *narrow = poly(r.q, NQ - 1, 2), *three = poly(r.q, NQ + NP, 3);
    lr_poly *keyq = poly(r.q, NQ, 1), *keylow = poly(r.q, NQ - 1, 1);
    std::vector<uint8_t> b((size_t)3 * N, 0);
    const uint8_t *u = b.data();
    // the form against the handle
    REFUSED(lr_ckks_encryptor_encrypt_pk(fast_only, 0, top, pk0, pk1, u, u, u, u, pt, 2, c0, c1) == LR_ERR_ARG);
    CHECK(std::string(lr_last_error_string()).find("fast form") != std::string::npos);
    REFUSED(lr_ckks_encryptor_encrypt_sk(fast_only, 0, top, sk, crp, u, pt, 2, c0, c1) == LR_ERR_ARG);
    OK(lr_ckks_encryptor_encrypt_pk(fast_only, 1, top, keyq, keyq, u, u, u, u, pt, 2, c0, c1));          // ... which serves the fast forms, keys over Q
    count += 2;
    // NULL arguments
    REFUSED(lr_ckks_encryptor_encrypt_pk(nullptr, 0, top, pk0, pk1, u, u, u, u, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_ckks_encryptor_encrypt_pk(enc, 0, top, nullptr, pk1, u, u, u, u, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_ckks_encryptor_encrypt_pk(enc, 0, top, pk0, pk1, nullptr, u, u, u, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_ckks_encryptor_encrypt_pk(enc, 0, top, pk0, pk1, u, u, u, nullptr, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_ckks_encryptor_encrypt_pk_device(enc, 0, top, pk0, pk1, u, nullptr, u, u, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_ckks_encryptor_encrypt_pk(enc, 0, top, pk0, pk1, u, u, u, u, nullptr, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_ckks_encryptor_encrypt_pk(enc, 0, top, pk0, pk1, u, u, u, u, pt, 2, c0, nullptr) == LR_ERR_ARG);
    REFUSED(lr_ckks_encryptor_encrypt_sk(enc, 0, top, nullptr, crp, u, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_ckks_encryptor_encrypt_sk(enc, 0, top, sk, nullptr, u, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_ckks_encryptor_encrypt_sk(enc, 0, top, sk, crp, nullptr, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_ckks_encryptor_encrypt_sk_device(enc, 0, top, sk, crp, nullptr, pt, 2, c0, c1) == LR_ERR_ARG);
    count += 11;
    // out_c0 == out_c1, a poly of another context, crp as an output
    REFUSED(lr_ckks_encryptor_encrypt_pk(enc, 0, top, pk0, pk1, u, u, u, u, pt, 2, c0, c0) == LR_ERR_ARG);
    REFUSED(lr_ckks_encryptor_encrypt_sk(enc, 1, top, sk, crp, u, pt, 2, c1, c1) == LR_ERR_ARG);
    REFUSED(lr_ckks_encryptor_encrypt_pk(enc, 0, top, foreign, pk1, u, u, u, u, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_ckks_encryptor_encrypt_pk(enc, 0, top, pk0, pk1, u, u, u, u, foreign, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_ckks_encryptor_encrypt_sk(enc, 0, top, sk, foreign, u, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_ckks_encryptor_encrypt_sk(enc, 0, top, sk, crp, u, pt, 2, foreign, c1) == LR_ERR_ARG);
    REFUSED(lr_ckks_encryptor_encrypt_sk(enc, 0, top, sk, crp, u, pt, 2, c0, crp) == LR_ERR_ARG);
    count += 7;
    // level
    REFUSED(lr_ckks_encryptor_encrypt_pk(enc, 0, -1, pk0, pk1, u, u, u, u, pt, 2, c0, c1) == LR_ERR_SHAPE);
    REFUSED(lr_ckks_encryptor_encrypt_pk(enc, 1, NQ, pk0, pk1, u, u, u, u, pt, 2, c0, c1) == LR_ERR_SHAPE);
    REFUSED(lr_ckks_encryptor_encrypt_sk(enc, 0, NQ, sk, crp, u, pt, 2, c0, c1) == LR_ERR_SHAPE);
    REFUSED(lr_ckks_encryptor_encrypt_sk_device(enc, 1, -1, sk, crp, u, pt, 2, c0, c1) == LR_ERR_SHAPE);
    count += 4;
    // batch and limbs
    REFUSED(lr_ckks_encryptor_encrypt_pk(enc, 0, top, pk0, pk1, u, u, u, u, pt, 0, c0, c1) == LR_ERR_SHAPE);
    REFUSED(lr_ckks_encryptor_encrypt_pk(enc, 0, top, pk0, pk1, u, u, u, u, three, 3, three, c1) == LR_ERR_SHAPE);   // above max_batch
    REFUSED(lr_ckks_encryptor_encrypt_pk(enc, 0, top, pk0, pk1, u, u, u, u, pt, 1, c0, c1) == LR_ERR_SHAPE);         // differs from the polys'
    REFUSED(lr_ckks_encryptor_encrypt_pk(enc, 0, top, three, pk1, u, u, u, u, pt, 2, c0, c1) == LR_ERR_SHAPE);
    REFUSED(lr_ckks_encryptor_encrypt_sk(enc, 0, top, sk, pk0, u, pt, 2, c0, c1) == LR_ERR_SHAPE);                   // crp of batch 1
    REFUSED(lr_ckks_encryptor_encrypt_pk(enc, 0, top, keyq, pk1, u, u, u, u, pt, 2, c0, c1) == LR_ERR_SHAPE);        // a key over Q for the form through P
    REFUSED(lr_ckks_encryptor_encrypt_pk(enc, 1, top, keylow, pk1, u, u, u, u, pt, 2, c0, c1) == LR_ERR_SHAPE);      // fewer than |Q| limbs for the fast form
    REFUSED(lr_ckks_encryptor_encrypt_pk(enc, 1, top, pk0, pk1, u, u, u, u, pt, 2, narrow, c1) == LR_ERR_SHAPE);     // fewer than level + 1 limbs
    REFUSED(lr_ckks_encryptor_encrypt_sk(enc, 1, top, sk, crp, u, narrow, 2, c0, c1) == LR_ERR_SHAPE);
    count += 9;
    OK(lr_ckks_encryptor_encrypt_pk(enc, 1, top - 1, pk0, pk1, u, u, u, u, narrow, 2, narrow, c1));                // ... which suffice one level down
    CHECK(launches() - before == 3 + 3);                                                                           // only the two accepted calls launched anything
    OK(lr_ckks_encryptor_encrypt_pk(enc, 0, top, pk0, pk1, u, u, u, u, pt, 2, c0, c1));                            // the handle stays usable
    for (lr_poly *p : {pk0, pk1, sk, crp, pt, c0, c1, foreign, narrow, three, keyq, keylow}) lr_poly_free(p);
    OK(lr_ckks_encryptor_destroy(fast_only));
    OK(lr_ckks_encryptor_destroy(enc));
    OK(lr_ckks_encryptor_destroy(nullptr));
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
        calls += exercise(N, nullptr);
        calls += exercise(N, &call_by_call);
    }
    sequences();
    refused += refusals();
    {   // two handles on two threads, each with its own contexts: nothing is shared but the library's globals
        std::atomic<int> threaded{0};
        std::thread a([&] { threaded += exercise(1 << 12, nullptr); });
        std::thread b([&] { threaded += exercise(1 << 4, &call_by_call); });
        a.join();
        b.join();
        calls += threaded.load();
    }
    return driver_end(ALLOCATIONS | EVENTS | LOG, refused, "ckks_encryptor: calls %d, refusals %d", calls, refused);
}
